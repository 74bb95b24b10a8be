"""The host side of the native estimate tool against its NumPy restatement (tools/estimate_restate.py): reading the
dumps, the ML update, the writers, the pool edits and the tool's refusals.  No device: plain --ml never opens one.

The restatement is the yardstick: the accumulated arrays and the estimated parameters are compared as
doubles with ==, the written files token for token against the restatement's values formatted "%g".  The pool-edit
fixtures have pairwise distinct occupancies and weights, so that no tie decides anything."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import estimate_restate as R  # noqa: E402

G, D, S = 12, 5, 4
MIXTURES = [([0, 1, 2, 3], [0.4, 0.3, 0.2, 0.1]), ([3, 4, 5], [0.5, 0.3, 0.2]), ([6, 7, 8], [0.2, 0.7, 0.1]),
            ([9, 10, 11], [0.25, 0.35, 0.4])]
HMMS = [("a", [0, 1]), ("b-c+d", [2, 3]), ("_", [1])]   # the last HMM ties its state to state 1
SELF = [0.6, 0.65, 0.7, 0.75]
N_TRANS = 8


def _exe(capi):
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "bin", "estimate")
    assert os.path.exists(exe), exe
    return exe


def _run(capi, *args):
    return subprocess.run([_exe(capi)] + list(args), capture_output=True, text=True)


def _model(base, seed=1):
    rng = np.random.default_rng(seed)
    R.write_model(base, rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, size=(G, D)), MIXTURES, HMMS, SELF)


def _ml_dumps(tmp, mode):
    """Three list entries.  Gaussian 11: no statistics anywhere; 10: one frame in one dump (feacount 1); 3: shared by
    mixtures 0 and 1; 7: so narrow in dimension 0 that --minvar floors it; mixture 3: no statistics; state 1: counts
    1000 and 0.4 (the 0.001 floor); state 3: no counts; the .phs of entry 2 ends after its count line."""
    rng = np.random.default_rng(10 + mode)
    full = mode == R.FULL
    bases = []
    for n in range(3):
        base = os.path.join(tmp, "dump%d_m%d" % (n, mode))
        gauss = [None] * G
        for g in range(G - 1):
            if g == 10 and n != 1:
                continue
            if (g + n) % 4 == 3 and g != 10:
                continue   # not every dump knows every Gaussian
            frames = 1 if g == 10 else int(rng.integers(5, 40))
            x = rng.normal(size=(frames, D)) * (0.5 + 0.1 * g) + g
            if g == 7:
                x[:, 0] = 7 + 0.01 * rng.normal(size=frames)
            gauss[g] = R.frame_statistics(x, rng.uniform(0.1, 1.0, size=frames), full)
        R.write_gks(base + ".gks", D, mode, gauss)
        mix = [(p, list(rng.uniform(1, 50, size=len(p))), -float(rng.uniform(10, 100))) if m != 3 and (m + n) % 3 != 2 else None
               for m, (p, _w) in enumerate(MIXTURES)]
        R.write_mcs(base + ".mcs", mode, mix)
        lines = [(0, 0, 30.5 + n), (0, 1, 11.25), (1, 0, 1000.0), (1, 1, 0.4 if n == 0 else 0.0), (2, 0, 7.0 + n), (2, 1, 3.0)]
        R.write_phs(base + ".phs", N_TRANS, [] if n == 2 else lines)
        R.write_lls(base + ".lls", [("Total log likelihood", -1234.5678 * (n + 1)), ("Number of frames", 100 + n)])
        bases.append(base)
    return bases


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("estimate"))
    _model(os.path.join(tmp, "prev"))
    return {"tmp": tmp, "prev": os.path.join(tmp, "prev"), 1: _ml_dumps(tmp, R.ML), 3: _ml_dumps(tmp, R.FULL)}


def _both(capi, work, mode, transitions=True):
    h, r = capi.Estimate.from_base(work["prev"]), R.Model(work["prev"])
    for b in work[mode]:
        h.add_dump(b, transitions)
        r.add_dump(b, transitions)
    return h, r


def _restated_statistics(r):
    xx = R.tri(D) if r.mode & 2 else D
    acc = np.array([r.accumulated(g) for g in range(G)], np.int32)
    get = lambda k, n: np.array([r.acc[g][k] if r.acc[g] is not None else ([0.0] * n if n else 0) for g in range(G)], np.float64)
    return acc, get("feacount", 0), get("gamma", 0), get("sum_x", D), get("sum_xx", xx)


@pytest.mark.parametrize("mode", [R.ML, R.FULL])
def test_accumulated_statistics_equal_the_restatement(capi, work, mode):
    h, r = _both(capi, work, mode)
    st = h.statistics()
    assert st["mode"] == mode == r.mode
    acc, fc, gamma, sx, sxx = _restated_statistics(r)
    assert not acc[11] and acc[10] and fc[10] == 1
    assert (st["accumulated"] == acc).all() and (st["feacount"] == fc).all()
    assert (st["gamma"] == gamma).all() and (st["sum_x"] == sx).all() and (st["sum_xx"] == sxx).all()
    assert st["sum_xx"].shape[1] == (R.tri(D) if mode == R.FULL else D)
    mg = np.concatenate([r.mix_acc[m]["gamma"] if r.mix_acc[m] is not None else [0.0] * len(MIXTURES[m][0]) for m in range(S)])
    assert (st["mix_gamma"] == mg).all()
    assert list(st["mix_accumulated"]) == [1, 1, 1, 0]
    assert (st["trans_occ"] == np.array(r.trans_acc)).all()
    assert list(st["trans_accumulated"]) == [int(a) for a in r.trans_accumulated]
    # the dumps list six of the eight transitions: the reader repeats the last line up to the announced count
    assert st["trans_occ"][5] == 2 * 3 * 3.0 and st["trans_occ"][6] == 0


@pytest.mark.parametrize("mode", [R.ML, R.FULL])
def test_ml_parameters_equal_the_restatement(capi, work, mode):
    h, r = _both(capi, work, mode)
    before = h.parameters()
    h.estimate_transitions()
    h.estimate_ml()
    r.estimate_transitions()
    r.estimate_gaussians()
    r.estimate_mixtures()
    p = h.parameters()
    assert (p["mean"] == np.array(r.mean)).all() and (p["var"] == np.array(r.var)).all()
    assert (p["mix_weight"] == np.concatenate(r.weights)).all()
    assert (p["trans_prob"] == np.array([t[2] for t in r.transitions])).all()
    assert p["var"][7, 0] == 0.1 and (p["var"][10] == 0.1).all()          # floored at --minvar
    assert (p["mean"][11] == before["mean"][11]).all() and (p["var"][11] == before["var"][11]).all()   # no statistics
    assert (p["mix_weight"][10:] == before["mix_weight"][10:]).all()      # the mixture without statistics
    assert p["trans_prob"][3] == 0.001                                      # the floor
    assert (p["trans_prob"][6:] == before["trans_prob"][6:]).all()         # the state without counts
    assert abs(p["mix_weight"][:4].sum() - 1) < 1e-12
    # --minvar as given
    h2, r2 = _both(capi, work, mode, False)
    h2.set_gaussian_parameters(0.5)
    r2.minvar = 0.5
    h2.estimate_ml(mixtures=False)
    r2.estimate_gaussians()
    p2 = h2.parameters()
    assert (p2["var"] == np.array(r2.var)).all() and p2["var"].min() == 0.5
    assert (p2["mix_weight"] == before["mix_weight"]).all()                # --no-mixture-update


def _tokens(path):
    return open(path).read().split()


def test_tool_writes_what_the_restatement_writes(capi, work):
    tmp = work["tmp"]
    lst = os.path.join(tmp, "list1")
    open(lst, "w").write("\n".join(work[1]) + "\n")
    out, summ = os.path.join(tmp, "out1"), os.path.join(tmp, "summary")
    open(summ, "w").write("earlier line\n")
    res = _run(capi, "-b", work["prev"], "-L", lst, "-o", out, "--ml", "-t", "-s", summ)
    assert res.returncode == 0, res.stderr
    assert "Could not estimate Gaussian parameters due to missing statistics" in res.stderr
    assert "Could not estimate mixture parameters due to missing statistics" in res.stderr
    r = R.Model(work["prev"])
    for b in work[1]:
        r.add_dump(b, True)
    r.estimate_transitions()
    r.estimate_gaussians()
    r.estimate_mixtures()
    assert _tokens(out + ".gk") == r.gk_tokens()
    assert _tokens(out + ".mc") == r.mc_tokens()
    assert _tokens(out + ".ph") == r.ph_tokens()
    assert not os.path.exists(out + ".cfg")
    assert open(summ).read().splitlines() == ["earlier line"] + r.summary_lines(work["prev"])
    # what was written is a model: it reads back to the written digits
    back = capi.Estimate.from_base(out).parameters()
    assert np.allclose(back["var"], np.array(r.var), rtol=1e-5) and np.allclose(back["trans_prob"], [t[2] for t in r.transitions], rtol=1e-5)
    # -g / -m / -p name the .gk in the summary; --no-mixture-update keeps the weights
    out2 = os.path.join(tmp, "out2")
    res = _run(capi, "-g", work["prev"] + ".gk", "-m", work["prev"] + ".mc", "-p", work["prev"] + ".ph", "-L", lst, "-o", out2,
               "--ml", "--no-mixture-update", "--minvar", "0.5", "--covsmooth", "2", "-s", summ)
    assert res.returncode == 0, res.stderr
    assert open(summ).read().splitlines()[-3] == work["prev"] + ".gk"
    r2 = R.Model(work["prev"])
    r2.minvar = 0.5
    for b in work[1]:
        r2.add_dump(b)
    r2.estimate_gaussians()
    assert _tokens(out2 + ".gk") == r2.gk_tokens() and _tokens(out2 + ".mc") == r2.mc_tokens()
    assert _tokens(out2 + ".ph") == r2.ph_tokens()     # without -t the transitions stay


def test_no_write_writes_nothing(capi, work):
    tmp = work["tmp"]
    lst = os.path.join(tmp, "list_nw")
    open(lst, "w").write("\n".join(work[3]) + "\n")
    out, summ = os.path.join(tmp, "out_nw"), os.path.join(tmp, "summary_nw")
    res = _run(capi, "-b", work["prev"], "-L", lst, "-o", out, "--ml", "--no-write", "-s", summ)
    assert res.returncode == 0, res.stderr
    assert not any(os.path.exists(out + e) for e in (".gk", ".mc", ".ph", ".cfg")) and not os.path.exists(summ)


REFUSED = [["--mmi"], ["--mpe"], ["--ml", "--C1", "1"], ["--ml", "--C2", "1"], ["--ml", "--ismooth", "1"],
           ["--ml", "--mmi-prior-ismooth", "1"], ["--ml", "--prev-prior"], ["--ml", "--limit", "1"],
           ["--ml", "--silence-d", "1"], ["--ml", "-D", "x"], ["--ml", "--write-ebwd", "x"], ["--ml", "-C", "x"],
           ["--ml", "--hcl-bfgs-cfg", "x"], ["--ml", "--hcl-line-cfg", "x"], ["--ml", "--no-silence-update"]]


@pytest.mark.parametrize("args", REFUSED, ids=lambda a: a[-2] if a[-1] in "1x" else a[-1])
def test_refused_options_name_themselves(capi, work, args):
    # nothing is read: neither the model nor the list exists
    res = _run(capi, "-b", "/nonexistent/model", "-L", "/nonexistent/list", "-o", os.path.join(work["tmp"], "never"), *args)
    assert res.returncode != 0
    name = args[0] if len(args) == 1 else args[1]
    assert name in res.stderr and "not supported" in res.stderr, res.stderr
    assert "nonexistent" not in res.stderr


def test_kept_messages_and_pool_refusal(capi, work):
    tmp = work["tmp"]
    lst = os.path.join(tmp, "list1k")
    open(lst, "w").write("\n".join(work[1]) + "\n")
    common = ["-b", work["prev"], "-L", lst, "-o", os.path.join(tmp, "never")]
    for extra in ([], ["--ml", "--mmi"], ["--ml", "--mpe"]):
        res = _run(capi, *common, *extra)
        assert res.returncode != 0 and "Define exactly one of --ml, --mmi and --mpe!" in res.stderr
    res = _run(capi, *common, "--ml", "--split")
    assert res.returncode != 0 and "Either --minocc or --numgauss is required with --split" in res.stderr
    res = _run(capi, *common, "--ml", "--mllt", "transform")
    assert res.returncode != 0 and "Must specify configuration file with MLLT" in res.stderr
    res = _run(capi, "-g", work["prev"] + ".gk", "-L", lst, "-o", os.path.join(tmp, "never"), "--ml")
    assert res.returncode != 0 and "Must give either --base or all --gk, --mc and --ph" in res.stderr
    assert not os.path.exists(os.path.join(tmp, "never.gk"))
    # pools with full-covariance Gaussians, by the tool and by the handle
    full = os.path.join(tmp, "fullpool")
    for e in (".mc", ".ph"):
        open(full + e, "w").write(open(work["prev"] + e).read())
    lines = open(work["prev"] + ".gk").read().splitlines()
    lines[1] = "full " + " ".join(["0"] * D + ["1" if i == j else "0" for i in range(D) for j in range(D)])
    open(full + ".gk", "w").write("\n".join(lines) + "\n")
    res = _run(capi, "-b", full, "-L", lst, "-o", os.path.join(tmp, "never"), "--ml")
    assert res.returncode != 0 and "only diagonal Gaussians are supported" in res.stderr
    with pytest.raises(capi.AasrError) as ei:
        capi.Estimate.from_base(full)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "diagonal" in ei.value.msg


def _copy_dump(src, dst, skip=()):
    for e in (".gks", ".mcs", ".phs", ".lls"):
        if e not in skip:
            open(dst + e, "wb").write(open(src + e, "rb").read())


def test_dump_errors(capi, work):
    tmp, good = work["tmp"], work[1][0]
    gks = open(good + ".gks", "rb").read()
    mcs, phs = open(good + ".mcs").read(), open(good + ".phs").read()

    def fails(ext, content, message, transitions=True):
        bad = os.path.join(tmp, "bad")
        _copy_dump(good, bad)
        open(bad + ext, "wb").write(content if isinstance(content, bytes) else content.encode())
        with pytest.raises(capi.AasrError) as ei:
            capi.Estimate.from_base(work["prev"]).add_dump(bad, transitions)
        assert message in ei.value.msg, ei.value.msg

    fails(".gks", struct.pack("<i", G + 1) + gks[4:], "the number of mixture base distributions in")
    fails(".gks", gks[:4] + struct.pack("<i", D + 1) + gks[8:], "the dimensionality of mixture base distributions in")
    fails(".gks", gks[:12] + struct.pack("<i", G), "Invalid statistics dump (wrong pdf index)")
    fails(".gks", gks[:12] + struct.pack("<i", -2), "Invalid statistics dump (wrong pdf index)")
    fails(".gks", gks[:12] + struct.pack("<iiidd", 0, 0, -1, 1.0, 0.0) + bytes(8 * D) + struct.pack("<i", -1), "Invalid statistics dump")
    fails(".gks", gks[:12] + struct.pack("<ii", 0, 1), "Invalid accumulator position 1")
    fails(".gks", gks[:8] + struct.pack("<i", 5) + gks[12:], "only ML statistics")
    fails(".mcs", "%d\n1\n" % (S + 1), "the number of PDFs in")
    fails(".phs", "%d\n" % (N_TRANS + 1), "the number of transitions in")
    fails(".phs", "%d\n0 0 1.5\n0 5 2.5\n" % N_TRANS, "the transition 1 could not be accumulated")
    # a missing .phs is only a message; without -t it is not even opened
    nophs = os.path.join(tmp, "nophs")
    _copy_dump(good, nophs, skip=(".phs",))
    h = capi.Estimate.from_base(work["prev"])
    h.add_dump(nophs, True)
    assert not h.statistics()["trans_accumulated"].any() and h.statistics()["accumulated"].any()
    with pytest.raises(capi.AasrError) as ei:
        capi.Estimate.from_base(work["prev"]).add_dump(os.path.join(tmp, "nowhere"))
    assert ei.value.code == capi.AASR_ERR_IO and "could not open" in ei.value.msg
    assert phs and mcs


# ---- the pool edits ---------------------------------------------------------------------------------

def _edit_case(tmp, name, occ, mix_gamma, weights=None):
    """A model of 12 Gaussians and 4 mixtures with statistics for all of them: Gaussian g has occupancy occ[g],
    mixture m the component occupancies mix_gamma[m].  -> the model's base and the dump's"""
    rng = np.random.default_rng(77)
    base, dump = os.path.join(tmp, name), os.path.join(tmp, name + "_dump")
    mixtures = [(p, w if weights is None else weights[m]) for m, (p, w) in enumerate(MIXTURES)]
    R.write_model(base, rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, size=(G, D)), mixtures, HMMS, SELF)
    gauss = []
    for g in range(G):
        frames = 20
        x = rng.normal(size=(frames, D)) + g
        gam = rng.uniform(0.5, 1.0, size=frames)
        gauss.append(R.frame_statistics(x, gam * (occ[g] / gam.sum()), False))
    R.write_gks(dump + ".gks", D, R.ML, gauss)
    R.write_mcs(dump + ".mcs", R.ML, [(p, mix_gamma[m], -50.0) for m, (p, _w) in enumerate(MIXTURES)])
    return base, dump


def _edited(capi, base, dump, ml=True):
    h, r = capi.Estimate.from_base(base), R.Model(base)
    h.add_dump(dump)
    r.add_dump(dump)
    if ml:
        h.estimate_ml()
        r.estimate_gaussians()
        r.estimate_mixtures()
    return h, r


def _same_model(h, r):
    p = h.parameters()
    assert p["mean"].shape == (len(r.mean), D)
    assert (p["mean"] == np.array(r.mean)).all() and (p["var"] == np.array(r.var)).all()
    assert list(p["mix_offsets"]) == list(np.cumsum([0] + [len(x) for x in r.pointers]))
    assert list(p["mix_index"]) == [x for ptr in r.pointers for x in ptr]
    assert (p["mix_weight"] == np.array([x for w in r.weights for x in w])).all()


OCC = [310.0, 95.5, 41.25, 220.0, 12.5, 150.75, 64.0, 480.5, 33.0, 5.5, 9.25, 7.75]
MIXG = [[120.0, 95.5, 41.25, 100.5], [119.5, 12.5, 150.75], [64.0, 480.5, 33.0], [5.5, 9.25, 7.75]]


def test_delete_keeps_the_heaviest_component(capi, tmp_path):
    base, dump = _edit_case(str(tmp_path), "del", OCC, MIXG)
    h, r = _edited(capi, base, dump)
    imap, n = h.delete_gaussians(40.0)
    want = r.delete_gaussians(40.0)
    # mixture 3 would lose 9, 10 and 11: the heaviest component (10) stays
    assert list(imap) == want and want[9] == -1 and want[10] >= 0 and want[11] == -1 and want[4] == -1 and want[8] == -1
    assert n == 4 and h.sizes()["gaussians"] == G - 4
    _same_model(h, r)
    assert list(h.parameters()["mix_weight"][-1:]) == [1.0]


def test_mremove_drops_unreferenced_gaussians(capi, tmp_path):
    base, dump = _edit_case(str(tmp_path), "mrm", OCC, MIXG)
    h, r = _edited(capi, base, dump)
    imap, n = h.remove_mixture_components(0.06)
    want = r.remove_mixture_components(0.06)
    # Gaussian 4 (weight 12.5 / 282.75 in mixture 1) and 8 leave their only mixture and the pool; 3 loses nothing
    assert list(imap) == want and want[4] == -1 and want[8] == -1 and n == want.count(-1) >= 2
    _same_model(h, r)


@pytest.mark.parametrize("kw, expect", [
    (dict(minocc=60.0, maxmixgauss=8), "some"),
    (dict(minocc=60.0), "none"),                               # --maxmixgauss defaults to 0: nothing may grow
    (dict(numgauss=17, maxmixgauss=8), "search"),
    (dict(minocc=20.0, maxmixgauss=4), "maxmix"),
    (dict(numgauss=20, maxmixgauss=8, splitalpha=0.5), "search"),
], ids=["minocc", "minocc-default-maxmix", "numgauss", "maxmixgauss-binds", "numgauss-alpha"])
def test_split(capi, tmp_path, kw, expect):
    base, dump = _edit_case(str(tmp_path), "split", OCC, MIXG)
    h, r = _edited(capi, base, dump)
    n = h.split_gaussians(**kw)
    args = dict(minocc=kw.get("minocc", 0.0), maxg=kw.get("maxmixgauss", 0), numgauss=kw.get("numgauss", -1),
                splitalpha=kw.get("splitalpha", 1.0))
    want, limit, steps = r.split_gaussians(**args)
    assert n == want
    _same_model(h, r)
    if expect == "none":
        assert n == 0
    else:
        assert n > 0 and h.sizes()["gaussians"] == G + n
    if expect == "search":
        assert steps > 1 and limit > 0
    if expect == "maxmix":
        sizes = np.diff(h.parameters()["mix_offsets"])
        assert sizes.max() == 4 and list(sizes[:1]) == [4]      # mixture 0 was full: its Gaussians did not split
    # the order of the tool: delete, remove, split
    h2, r2 = _edited(capi, base, dump)
    h2.delete_gaussians(8.0)
    r2.delete_gaussians(8.0)
    h2.remove_mixture_components(0.05)
    r2.remove_mixture_components(0.05)
    assert h2.split_gaussians(**kw) == r2.split_gaussians(**args)[0]
    _same_model(h2, r2)


def test_tool_edits_in_the_reference_order(capi, tmp_path):
    base, dump = _edit_case(str(tmp_path), "tooledit", OCC, MIXG)
    lst, out = str(tmp_path / "list"), str(tmp_path / "out")
    open(lst, "w").write(dump + "\n")
    res = _run(capi, "-b", base, "-L", lst, "-o", out, "--ml", "--delete", "8", "--mremove", "0.05", "--split", "--minocc", "60",
               "--maxmixgauss", "8", "-i", "1")
    assert res.returncode == 0, res.stderr
    _h, r = _edited(capi, base, dump)
    r.delete_gaussians(8.0)
    r.remove_mixture_components(0.05)
    n = r.split_gaussians(60.0, 8)[0]
    assert "Split %d Gaussians" % n in res.stdout and n > 0
    assert _tokens(out + ".gk") == r.gk_tokens() and _tokens(out + ".mc") == r.mc_tokens()


# ---- the MLLT row solver ----------------------------------------------------------------------------

def test_mllt_row_solver(capi):
    """One inner update of aku/HmmSet.cc:955-980 on a 5 x 5 case.  The native solver and the restatement take the same
    cofactors c_i = |det A| (A^T)^-1 and differ only by their inverse's rounding, which perturbs the result by a
    multiple of cond(A) 2^-53: the bound is 64 cond(A) 2^-53 relative to the largest entry."""
    rng = np.random.default_rng(5)
    d = 5
    A = np.eye(d) + 0.2 * rng.normal(size=(d, d))
    g_inv = np.empty((d, d, d))
    for i in range(d):
        B = rng.normal(size=(d, 3 * d))
        g_inv[i] = np.linalg.inv(B @ B.T / (3 * d) + 0.5 * np.eye(d))
    beta = 1234.5
    got = capi.mllt_update_rows(A, g_inv, beta, 1)
    want = R.update_rows(A, g_inv, beta, 1)
    bound = 64 * np.linalg.cond(A) * 2.0 ** -53
    err = np.abs(got - want).max() / np.abs(want).max()
    print("row solver: relative difference %.3g, bound %.3g" % (err, bound))
    assert err <= bound
    # every row comes from the PREVIOUS A: updating row after row gives another matrix
    seq = A.copy()
    for i in range(d):
        At = seq.T.copy()
        c = abs(np.linalg.det(At)) * np.linalg.inv(At)[i]
        row = g_inv[i].T @ c
        seq[i] = row * np.sqrt(beta / (c @ row))
    assert np.abs(seq - want).max() > 1e-6 * np.abs(want).max()

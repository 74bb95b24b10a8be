"""FST decoder confidence, host side (no GPU): the restatement tools/fst_conf_restate.py against the reference's recorded
answers (tests/golden/fst_conf/expected_conf_*.txt, written by tools/make_fst_conf_golden.py), its parts against brute
force and hand cases, the host's own junk removal, edit distance and formulas (csrc/fst_conf.cc) against the
restatement, the ABI, the refusals before a device is needed, the module's surface and the tool's options."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fst_restate as R  # noqa: E402
import fst_conf_restate as CR  # noqa: E402

FST = os.path.join(ROOT, "tests", "golden", "fst")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fst_conf")
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
CASES = sorted(os.path.basename(p)[14:-4] for p in glob.glob(os.path.join(GOLDEN, "expected_conf_*.txt")))
FIELDS = ("token_conf", "ploop_conf", "edit_conf", "best_acu_conf", "grammar_logprob", "ploop_logprob", "best_final_logprob",
          "best_different_logprob", "best_acu_score")


def g9(x) -> bytes:
    return ("%.9g" % float(x)).encode()


def bits(x) -> bytes:
    return np.float32(x).tobytes()


def expected(case):
    """rows of (grammar options, phone options, the 15 recorded fields behind the settings)"""
    rows = []
    for line in open(os.path.join(GOLDEN, "expected_conf_%s.txt" % case), "rb").read().split(b"\n"):
        if line:
            f = line.split(b"\t")
            g = dict(beam=float(f[0]), token_limit=int(f[1]), duration_scale=float(f[2]), transition_scale=float(f[3]))
            p = dict(beam=float(f[4]), token_limit=int(f[5]), duration_scale=float(f[6]), transition_scale=1.0)
            rows.append((g, p, f[7:]))
    return rows


def load_case(case):
    net = R.read_fst(open(os.path.join(FST, case + ".fst"), "rb").read())
    pnet = R.read_fst(open(os.path.join(GOLDEN, case + ".ploop.fst"), "rb").read())
    ac, lnabytes = R.read_lna(os.path.join(FST, case + ".lna"))
    return net, pnet, ac, lnabytes, R.read_durations(open(os.path.join(FST, case + ".dur")).read())


def recorded(c, plain, frames):
    return [c.text, c.ploop_text] + [g9(c.r[k]) for k in FIELDS] + [b"%d" % frames, g9(c.r["confidence"]), g9(plain.r["confidence"])]


def test_the_golden_cases_are_there():
    assert CASES == ["durhi", "rand1", "rand2", "rand4", "toy"]
    assert {load_case(c)[3] for c in CASES} == {1, 2, 4}
    rows = [f for c in CASES for _, _, f in expected(c)]
    tok, edit = [float(f[2]) for f in rows], [float(f[4]) for f in rows]
    for c in CASES:      # what the maker asserted of its rows
        assert any(0 < float(f[2]) < 1 for _, _, f in expected(c)), c
    assert 0.0 in tok and 1.0 in tok and any(0 < e < 1 for e in edit)
    assert any(f[9] == b"-10000000" for f in rows)      # a row with one hypothesis only: the sentinel


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    """both strings and every %.9g field (which identifies a float), and no tie in either search"""
    net, pnet, ac, _, dur = load_case(case)
    for g, p, f in expected(case):
        c = CR.confidence(net, ac, g, dur, pnet, p)
        plain = CR.confidence(net, ac, g, dur)
        assert c.ties == [] and plain.ties == [] and not c.no_final
        assert recorded(c, plain, ac.shape[0]) == f, (case, g, p)
        assert plain.r["best_acu_score"] == 0 and plain.r["ploop_conf"] == 0 and plain.r["edit_conf"] == 0


def test_best_different_equals_a_brute_force_scan():
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(300):
        n = int(rng.integers(0, 9))
        lps = sorted((np.float32(-rng.integers(0, 12) / 4.0) for _ in range(n)), reverse=True)
        tokens = [(int(rng.integers(0, 4)), lp, 1, tuple(int(w) for w in rng.integers(0, 2, int(rng.integers(0, 3))))) for lp in lps]
        end = [0, int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0]
        has_final, words, bf, bd, has_diff = CR.best_different(tokens, end)
        finals = [i for i, t in enumerate(tokens) if end[t[0]]]
        if not finals:
            assert (has_final, bits(bf), bits(bd), has_diff) == (False, bits(-9999999.9), bits(-9999999.9), False)
            seen.add("none")
            continue
        best = min(finals, key=lambda i: (-float(tokens[i][1]), i))
        others = [float(t[1]) for t in tokens if t[3] != tokens[best][3]]
        assert has_final and words == tokens[best][3] and bits(bf) == bits(tokens[best][1])
        assert has_diff == bool(others) and bits(bd) == bits(max(others) if others else -9999999.9)
        seen.add("diff" if others else "alone")
        seen.add("above" if others and max(others) > float(bf) else "below")
    assert seen == {"none", "diff", "alone", "above", "below"}


JUNK = [(b"", b""), (b"   ", b""), (b"aaaa", b"a"), (b"a a a", b"a"), (b"ab ba", b"aba"), (b"a  bb c", b"abc"),
        (b"\xe4\xe4 \xe4ni", b"\xe4ni"), (b"hello world", b"helo world".replace(b" ", b""))]
DIST = [(b"", b"", 0), (b"", b"abc", 3), (b"abc", b"", 3), (b"aaaa", b"aaaa", 0), (b"aaaa", b"aa", 2), (b"kitten", b"sitting", 3),
        (b"\xe4ni", b"ani", 1), (b"abc", b"cab", 2), (b"flaw", b"lawn", 2)]


def test_junk_removal_and_edit_distance_on_hand_cases(capi):
    for s, want in JUNK:
        assert CR.remove_junk(s) == want and capi.fst_conf_remove_junk(s) == want, s
    for a, b, d in DIST:
        assert CR.edit_distance(a, b) == d == capi.fst_conf_edit_distance(a, b), (a, b)
        assert CR.edit_distance(b, a) == d
    rng = np.random.default_rng(0)
    for _ in range(100):
        a, b = (bytes(rng.integers(97, 100, int(rng.integers(0, 9))).astype(np.uint8)) for _ in range(2))
        assert CR.edit_distance(a, b) == capi.fst_conf_edit_distance(a, b)


def test_host_formulas_equal_the_restatement_bitwise(capi):
    """csrc/fst_conf.cc on given inputs: ordinary values, both clamps, the empty result, zero frames, an empty cleaned string"""
    cases = [(9, -7.87, -21.6, -7.87, -8.82, -25.15, 1, b"world", b"l i h"),
             (20, -30.5, -28.25, -30.5, -9999999.9, -12.0, 2, b"w1 w3", b"w 1 3"),
             (20, -30.5, -28.25, -30.5, -20.0, -12.0, 2, b"w1 w3", b"3 w"),
             (12, -5.0, -6.0, -5.0, -5.5, -4.0, 0, b"", b"a"),          # no words: "Emptiness"
             (12, -1.0, -6.0, -9999999.9, -9999999.9, -4.0, 0, b"", b""),   # no end-node token; 0 / 0 in the edit term
             (0, 0.0, 0.0, 0.0, -9999999.9, 0.0, 1, b"a", b"a"),         # zero frames: the division's IEEE result
             (0, -1.0, -2.0, -1.0, -3.0, 0.0, 1, b"a", b"b"),
             (7, -3.0, -3.5, -3.0, -2.0, -2.5, 3, b"aa bb", b"a b")]
    for frames, glp, plp, bf, bd, acu, nw, gs, ps in cases:
        f = np.float32
        inputs = dict(frames=frames, grammar_logprob=glp, ploop_logprob=plp, best_final_logprob=bf, best_different_logprob=bd, best_acu_score=acu)
        for ploop in (ps, None):
            want = CR.formulas(frames, f(glp), f(plp), f(bf), f(bd), f(acu), nw, gs, ploop)
            got = capi.fst_conf_formulas(inputs, nw, gs, ploop)
            for k in ("confidence", "token_conf", "ploop_conf", "edit_conf", "best_acu_conf"):
                assert bits(got[k]) == bits(want[k]) or (np.isnan(got[k]) and np.isnan(want[k])), (frames, k, got[k], want[k])
    assert CR.formulas(12, f(-1), f(-6), f(-9999999.9), f(-9999999.9), f(-4), 0, b"", b"")["edit_conf"] == 0      # max(0, NaN)


def test_frame_best_restatement():
    f = np.float32
    ac = np.array([[-3, -1, -2], [-np.inf, -np.inf, -np.inf], [-0.0, 0.0, -5], [0.0, -0.0, -5], [-2, -2, -2]], np.float32)
    b = CR.frame_best(ac)
    assert [bits(x) for x in b] == [bits(-1), bits(-999999999.9), bits(-0.0), bits(0.0), bits(-2)]
    assert bits(CR.frame_best_sum(ac[[0, 4]])) == bits(f(f(0) + f(-1)) + f(-2))


# ---- ABI, refusals, module, tool -------------------------------------------------------------------------------------

def test_abi_symbols_and_defaults(capi):
    names = set(capi.declared_symbols())
    need = {"aasr_fst_conf_default_options", "aasr_fst_conf_batch_create", "aasr_fst_conf_batch_destroy", "aasr_fst_conf_batch_dev",
            "aasr_fst_conf_batch_frame_best_dev", "aasr_fst_conf_batch_sync", "aasr_fst_conf_batch_result", "aasr_fst_conf_batch_grammar",
            "aasr_fst_conf_batch_phone", "aasr_fst_conf_batch_options", "aasr_fst_conf_batch_record", "aasr_fst_conf_batch_frame_best",
            "aasr_fst_confidence_default_options", "aasr_run_fst_confidence_recipe"}
    assert need <= names and all(hasattr(capi.lib(), n) for n in need)
    o = capi.FstConfOptions.defaults()
    for s in (o.grammar, o.phone):
        assert (s.beam, s.token_limit, s.duration_scale, s.transition_scale) == (2600.0, 5000, 3.0, 1.0)
        assert (s.dur_by_state, s.cap_candidates, s.cap_recomb, s.cap_history) == (0, 0, 0, 0)
    assert o.phone_loop == 0 and o.verbose == 0
    assert C.sizeof(capi.FstOptions) == 32 and C.sizeof(o) == 72
    t = capi.FstConfidenceOptions.defaults()
    assert t.phone.beam == 2600.0 and t.phone_loop == 0 and t.decode.group == 256 and t.decode.fst.token_limit == 5000


def test_create_refuses_before_the_device(capi):
    net = capi.FstNet(os.path.join(FST, "toy.fst"))
    T = np.array([3], np.int32)

    def create(grammar, phone, o):
        b = C.c_void_p()
        st = capi.lib().aasr_fst_conf_batch_create(grammar, phone, None, C.byref(o), 1, T.ctypes.data, C.byref(b))
        return st, capi.lib().aasr_last_error().decode(), b.value

    st, msg, h = create(None, None, capi.FstConfOptions.defaults())
    assert st == capi.AASR_ERR_INVALID and "grammar" in msg and not h
    o = capi.FstConfOptions.defaults(phone_loop=1)
    o.phone.beam = -1.0
    st, msg, h = create(net.handle, net.handle, o)
    assert st == capi.AASR_ERR_INVALID and "phone beam" in msg and not h
    o = capi.FstConfOptions.defaults()
    o.phone.duration_scale = float("nan")
    st, msg, h = create(net.handle, None, o)
    assert st == capi.AASR_ERR_INVALID and "phone scales" in msg and not h
    o = capi.FstConfOptions.defaults()
    o.grammar.transition_scale = float("nan")
    st, msg, h = create(net.handle, None, o)
    assert st == capi.AASR_ERR_INVALID and "grammar scales" in msg
    st, msg, h = create(net.handle, None, capi.FstConfOptions.defaults(phone_loop=1))
    assert st == capi.AASR_ERR_INVALID and "phone-loop network" in msg


SEARCH = ("set_beam", "set_token_limit", "set_duration_scale", "set_transition_scale", "get_beam", "get_token_limit",
          "get_duration_scale", "get_transition_scale", "lna_open", "lna_close", "init_search", "run", "get_result",
          "get_result_and_logprob", "get_best_token_logprob", "get_best_final_token_logprob", "best_tokens", "tokens_at_final_states")
CONF = ("set_logprob_conf_weight", "set_logprob_conf_hysteresis", "result_and_confidence")
PHONE = ("set_phone_beam", "set_phone_token_limit", "set_phone_duration_scale", "set_phone_loop_logprob_weight", "get_ploop_conf",
         "get_token_conf", "get_edit_conf", "get_best_acu_conf")


def test_module_has_the_confidence_classes(capi, tmp_path):
    from aaltoasr_amd import FstDecoder
    toy, dur = os.path.join(FST, "toy.fst"), os.path.join(FST, "toy.dur")
    c = FstDecoder.FstSearchC(toy, None, dur)
    p = FstDecoder.FstConfidence(toy, None, dur)
    w = FstDecoder.FstConfidenceWithPhoneLoop(toy, os.path.join(GOLDEN, "toy.ploop.fst"), None, dur)
    for obj, names in ((c, SEARCH), (p, SEARCH + CONF), (w, SEARCH + CONF + PHONE)):
        for name in names:
            assert callable(getattr(obj, name)), (type(obj).__name__, name)
    for obj in (c, p, w):
        assert (obj.get_beam(), obj.get_token_limit(), obj.get_duration_scale(), obj.get_transition_scale()) == (2600.0, 5000, 3.0, 1.0)
    w.set_phone_beam(40)
    w.set_phone_token_limit(50)
    w.set_phone_duration_scale(2)
    w.set_phone_loop_logprob_weight(0.5)
    w.set_logprob_conf_weight(3)
    w.set_logprob_conf_hysteresis(50)
    assert (w._phone_opt.beam, w._phone_opt.token_limit, w._phone_opt.duration_scale) == (40.0, 50, 2.0)
    assert w.get_beam() == 2600.0      # the grammar search keeps its own
    w.init_search()
    assert w.get_result() == b""
    with pytest.raises(RuntimeError, match="run"):
        w.result_and_confidence()
    with pytest.raises(RuntimeError, match="Unknown header"):
        FstDecoder.FstConfidenceWithPhoneLoop(toy, dur, None, None)
    assert "never consults the HMM file" in FstDecoder.__doc__ and "is not built" not in FstDecoder.__doc__


def tool(*args):
    return subprocess.run([os.path.join(BIN, "fst_decode")] + list(args), capture_output=True, timeout=300)


def test_tool_names_and_refuses_the_new_options(capi, tmp_path):
    r = tool("--help")
    text = r.stdout + r.stderr
    for name in (b"--confidence", b"--phone-loop", b"--phone-beam", b"--phone-token-limit", b"--phone-duration-scale"):
        assert name in text, name
    rec = str(tmp_path / "r.recipe")
    open(rec, "w").write("lna=%s\n" % os.path.join(FST, "toy.lna"))
    out = str(tmp_path / "out.txt")
    common = ["--fst", os.path.join(FST, "toy.fst"), "-r", rec, "-o", out, "--lna-files"]
    for flags, word in ((["--phone-beam", "30"], b"--phone-beam without --confidence"),
                        (["--phone-loop", os.path.join(GOLDEN, "toy.ploop.fst")], b"--phone-loop without --confidence"),
                        (["--phone-token-limit", "3"], b"--phone-token-limit without --confidence"),
                        (["--phone-duration-scale", "1"], b"--phone-duration-scale without --confidence"),
                        (["--confidence", "--phone-beam", "30"], b"--phone-beam without --phone-loop"),
                        (["--confidence", "--phone-loop", os.path.join(GOLDEN, "toy.ploop.fst"), "--phone-beam", "-2"], b"phone beam")):
        r = tool(*common, *flags)
        assert r.returncode == 1 and r.stderr.startswith(b"exception: ") and word in r.stderr, (flags, r.stderr)
        assert not os.path.exists(out)


def test_kernel_notes(capi):
    """the confidence kernels from the code object: no scratch, no spills, LDS only in the token pass (csrc/fst_conf.h)"""
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "fst_conf.hip.o")
    assert os.path.exists(obj)
    notes = {k.split("::")[-1]: v for k, v in kernel_notes.kernel_notes(obj).items()}
    assert sorted(notes) == ["k_fst_conf_tokens", "k_fst_frame_best<1>", "k_fst_frame_best<2>", "k_fst_frame_best<4>", "k_fst_frame_sum"], sorted(notes)
    for name, k in notes.items():
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["vgpr"] <= 64, (name, k)
        assert k["lds"] == (48 if name == "k_fst_conf_tokens" else 0), (name, k)

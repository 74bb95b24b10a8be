"""State tying, the host side (no GPU): labels, the rule file, the replay of the split loop's cluster order, the basebind
bytes, the tool's messages -- every one of them comes before the device is opened -- and the loud failure without one.

Yardstick: tools/tie_restate.py (aku/tie.cc over aku/PhonePool.cc in NumPy) and bytes written out by hand."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TR = _load("tie_restate")


@pytest.mark.parametrize("label,want", [
    ("a-b+c", ("b", ["a"], ["c"])),
    ("x-a-b+c+y", ("b", ["a", "x"], ["c", "y"])),          # nearest context first on both sides
    ("b", ("b", [], [])),
    ("_", ("_", [], [])),
    ("a-b", ("b", ["a"], [])),
    ("b+c", ("b", [], ["c"])),
    ("aa-bcd+ee", ("bcd", ["aa"], ["ee"])),
])
def test_labels(capi, label, want):
    assert capi.tie_parse_label(label) == want
    assert (TR.center_phone(label), TR.left_contexts(label), TR.right_contexts(label)) == want


def test_label_without_a_centre_is_the_reference_error(capi):
    with pytest.raises(capi.AasrError) as ei:
        capi.tie_parse_label("a-+c")
    assert ei.value.code == capi.AASR_ERR_INVALID and ei.value.msg == "PhonePool: Invalid phone labela-+c"
    with pytest.raises(ValueError):
        TR.center_phone("a-+c")


def test_rule_file(capi, tmp_path):
    text = "R_ab context a,b\n\nL_c\tCONTEXT  c\nmixed CoNtExT b, a ,d\n"
    p = tmp_path / "ok.rules"
    p.write_text(text)
    t = capi.Tie(3, str(p))
    assert t.rules() == [("R_ab", ["a", "b"]), ("L_c", ["c"]), ("mixed", ["a", "b", "d"])]    # phones in set order
    assert [(n, sorted(s)) for n, s in TR.read_rules(text)] == t.rules()
    for bad, message in (("only_a_name\n", "PhonePool::load_decision_tree_rules: Invalid rule line:\nonly_a_name"),
                         ("r question a,b\n", "PhonePool::load_decision_tree_rules: Invalid rule type question"),
                         ("r CONTEXT\n", "PhonePool::load_decision_tree_rules: No phones in the context rule:\nr CONTEXT")):
        q = tmp_path / "bad.rules"
        q.write_text(bad)
        with pytest.raises(capi.AasrError) as ei:
            capi.Tie(3, str(q))
        assert ei.value.code == capi.AASR_ERR_INVALID and ei.value.msg == message
        with pytest.raises(ValueError):
            TR.read_rules(bad)
    with pytest.raises(capi.AasrError) as ei:
        capi.Tie(3, str(tmp_path / "none.rules"))
    assert ei.value.code == capi.AASR_ERR_IO
    with pytest.raises(capi.AasrError) as ei:
        capi.Tie(64, str(p))
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED and "1 ... 63" in ei.value.msg


def test_basebind_bytes_worked_by_hand(capi, tmp_path):
    """Contexts a and b; the phone _ (one state, written plain), k (one state, four context phones) and t (two states,
    one context phone).  Ten frames each, --count 10, --sgain 2, rules A = {a}, B = {b}.

    k's root {a-k+a, a-k+b, b-k+a, b-k+b}: A at -1 takes the smaller-or-equal yes side {a-k+a, a-k+b} (gain 5), A at +1
    {a-k+a, b-k+a} (3), B at -1 {b-k+a, b-k+b} (5: no strict lead, the first stays), B at +1 {a-k+b, b-k+b} (1).  The
    split cluster is looked at again: its halves of one member each gain 1 and 0.5, under --sgain.  The other half
    {b-k+a, b-k+b} splits by A at +1 (gain 4) into {b-k+a} and, appended, {b-k+b}.  States: _ 0; k 1 2 3; t 4 5."""
    p = tmp_path / "ab.rules"
    p.write_text("A context a\nB context b\n")
    t = capi.Tie(2, str(p))
    pool = TR.Pool(TR.read_rules(p.read_text()))
    labels = [("t", "a-t+b", 0), ("k", "a-k+a", 0), ("k", "a-k+b", 0), ("_", "_", 0), ("k", "b-k+a", 0), ("k", "b-k+b", 0),
              ("t", "a-t+b", 1)]
    cls = {}
    for _ph, lab, st in labels:
        cls[(lab, st)] = t.context_phone(lab, st)
        assert pool.context_phone(lab, st) == cls[(lab, st)]
    assert t.context_phone("a-k+b", 0) == cls[("a-k+b", 0)] and t.num_classes() == 7     # known: the same class
    table = {("a-k+a", "a-k+b"): 5.0, ("a-k+a", "b-k+a"): 3.0, ("b-k+a", "b-k+b"): 5.0, ("a-k+b", "b-k+b"): 1.0,
             ("a-k+a",): 1.0, ("a-k+b",): 0.5, ("b-k+a",): 4.0, ("b-k+b",): 4.0}
    name = {v: k[0] for k, v in cls.items()}

    def gain_of(_members, new):
        return table[tuple(sorted(name[c] for c in new))]

    t.set_occupancy(np.full(7, 10.0))
    t.split_given(gain_of, count=10, sgain=2.0, context=1)
    want = (b"_ 1 0\na-k+a 1 1\na-k+b 1 1\nb-k+a 1 2\nb-k+b 1 3\n"
            b"a-t+a 2 4 5\na-t+b 2 4 5\nb-t+a 2 4 5\nb-t+b 2 4 5\n")
    assert t.basebind(1) == want
    out = tmp_path / "o.basebind"
    t.write_basebind(str(out), 1)
    assert out.read_bytes() == want
    assert t.basebind(0) == b"_ 1 0\nk 1 1\nt 2 4 5\n"          # --context 0: every phone plain, its first clusters
    got = t.clusters()
    assert [(c["phone"], c["state"], c["index"], c["members"]) for c in got] == [
        ("_", 0, 0, [cls[("_", 0)]]), ("k", 0, 1, [cls[("a-k+a", 0)], cls[("a-k+b", 0)]]), ("k", 0, 2, [cls[("b-k+a", 0)]]),
        ("k", 0, 3, [cls[("b-k+b", 0)]]), ("t", 0, 4, [cls[("a-t+b", 0)]]), ("t", 1, 5, [cls[("a-t+b", 1)]])]
    assert got[1]["rules"] == [[("A", -1, True)]] and got[2]["rules"] == [[("A", -1, False), ("A", 1, True)]]
    assert got[3]["rules"] == [[("A", -1, False), ("A", 1, False)]] and got[0]["rules"] == [] and got[1]["occ"] == 20.0
    res = TR.split(pool, [10.0] * 7, 10, 2.0, 1, gain_of)
    assert TR.basebind_bytes(pool, res, 1) == want and TR.final_clusters(pool, res) == got


def _five_phone_pool(capi, rules_path, rules_text, context_labels, two_contexts=False):
    t = capi.Tie(4, rules_path)
    pool = TR.Pool(TR.read_rules(rules_text))
    for ph in ("zz", "x", "_s", "y"):
        for l in context_labels:
            for r in context_labels:
                if (ph, l, r) in (("x", "a", "b"), ("y", "c", "c")):
                    continue                                    # context phones the data never showed
                label = "%s-%s+%s" % (l, ph, r)
                if two_contexts and ph == "x":
                    label = "%s-%s+%s" % (r, label, l)
                for s in range(1 if ph == "_s" else 3):
                    assert t.context_phone(label, s) == pool.context_phone(label, s)
    return t, pool


@pytest.mark.parametrize("context,two", [(1, False), (2, True), (0, True)])
def test_cluster_order_replay_against_the_restatement(capi, tmp_path, context, two):
    """Gains given by hand (a fixed function of the new set): the order in which clusters are split, split again and
    appended is the state numbering, and has to be the restatement's for any outcome of the comparisons -- negative
    gains, gains under --sgain, exact ties and a NaN among them."""
    text = "R_ab context a,b\nL_a Context a\nR_c CONTEXT c\nR_ba context b,a\nL_bc context b,c\nR_abc context a,b,c\n"
    p = tmp_path / "r.rules"
    p.write_text(text)
    t, pool = _five_phone_pool(capi, str(p), text, "abc_", two)
    n = t.num_classes()
    occ = np.random.default_rng(3).integers(0, 50, n).astype(np.float64)
    occ[5] = 0.0                                                # a context phone without frames is a member all the same

    def gain_of(_members, new):
        v = (sum(new) * 7919) % 1000
        if v % 17 == 0:
            return float("nan")
        return float(v // 10 * 10) / 10.0 - 20.0                # steps of one: ties happen

    t.set_occupancy(occ)
    t.split_given(gain_of, count=60, sgain=5.0, context=context)
    res = TR.split(pool, list(occ), 60, 5.0, context, gain_of)
    got, want = t.clusters(), TR.final_clusters(pool, res)
    assert got == want
    assert max(len(v) for v in res.values()) >= 4 and len({len(v) for v in res.values()}) > 1
    for ctx in (1, 2, 0):
        assert t.basebind(ctx) == TR.basebind_bytes(pool, res, ctx)


# ---- the tool's messages: before the device is opened (this runs without one) ---------------------------------------

CFG = "module\n{\n  name pre\n  type pre\n  dim 3\n}\n"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tie_host")
    open(str(d / "f.cfg"), "w").write(CFG)
    open(str(d / "r.rules"), "w").write("A context a\n")
    open(str(d / "ok.phn"), "w").write("0 1280 a-k+a.0\n1280 2560 a-k+b.0\n")
    open(str(d / "nostate.phn"), "w").write("0 1280 a-k+a.0\n1280 2560 a-k+b\n")
    open(str(d / "r.rcp"), "w").write("audio=%s transcript=%s\n" % (d / "none.fea", d / "ok.phn"))
    open(str(d / "nostate.rcp"), "w").write("audio=%s transcript=%s\n" % (d / "none.fea", d / "nostate.phn"))
    open(str(d / "lines.rcp"), "w").write("audio=a.fea transcript=%s start-line=3 end-line=5\n" % (d / "ok.phn"))
    open(str(d / "bad.rules"), "w").write("A question a\n")
    open(str(d / "model.spkc"), "w").write("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    return d


def run_tool(files, *extra, recipe="r.rcp", rules="r.rules", out=("-B", "o.basebind")):
    cmd = [os.path.join(BIN, "tie"), "-c", str(files / "f.cfg"), "-r", str(files / recipe), "-u", str(files / rules)]
    cmd += [str(files / a) if not a.startswith("-") else a for a in out] + list(extra)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)


def test_tool_messages_come_before_the_device(capi, files):
    r = run_tool(files, "-H", recipe="none.rcp")                                    # before anything is read
    assert r.returncode == 1 and r.stderr == "exception: This feature is currently broken. Fix it?\n", r.stderr
    for out in ((), ("-B", "o.basebind", "-o", "o")):
        r = run_tool(files, out=out)
        assert r.returncode == 1 and r.stderr == "exception: Specify either --out or --basebind for output\n", r.stderr
    r = run_tool(files, recipe="nostate.rcp")
    assert r.returncode == 1 and r.stderr == "exception: Context phone tying requires phn files with state numbers!\n", r.stderr
    r = run_tool(files, recipe="lines.rcp")
    assert r.returncode == 1 and "tie: recipe line limits (start-line / end-line) are not supported" in r.stderr, r.stderr
    r = run_tool(files, rules="bad.rules")
    assert r.returncode == 1 and "PhonePool::load_decision_tree_rules: Invalid rule type question" in r.stderr, r.stderr
    r = run_tool(files, "-S", str(files / "model.spkc"))
    assert r.returncode == 1 and "speaker files with model transforms" in r.stderr, r.stderr
    r = run_tool(files, out=("-o", "o"), rules="none.rules")
    assert r.returncode == 1 and "could not open" in r.stderr, r.stderr
    assert not os.path.exists(str(files / "o.basebind")) and not os.path.exists(str(files / "o.gk"))


def test_tool_help_lists_the_reference_options(capi):
    r = subprocess.run([os.path.join(BIN, "tie"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: tie [OPTION...]\n")
    for opt in ("-c, --config=FILE", "-r, --recipe=FILE", "-O, --ophn", "-H, --hmmnet", "-b, --base=BASENAME", "-C, --mconfig=FILE",
                "-u, --rule=FILE", "-o, --out=FILE", "-B, --basebind=FILE", "--count=INT", "--sgain=FLOAT", "--mloss=FLOAT",
                "--context=INT", "-F, --fw-beam=FLOAT", "-W, --bw-beam=FLOAT", "-A, --ac-scale=FLOAT", "-V, --vit",
                "-S, --speakers=FILE", "-i, --info=INT", "--device=INT"):
        assert opt in r.stdout, opt


def test_an_accepted_command_line_reaches_the_device_and_fails_there(capi, files):
    """the counterpart of the refusals: what is not refused goes on to open the device, and says so when there is none"""
    r = run_tool(files)
    assert r.returncode == 1 and "tie:" not in r.stderr and "no HIP device available" in r.stderr, r.stderr
    assert "no CPU fallback" in r.stderr


def test_library_has_no_cpu_fallback(capi, files):
    """the step entries that compute need the device: without one each is AASR_ERR_NO_DEVICE"""
    t = capi.Tie(3, str(files / "r.rules"))
    for lab in ("a-k+a", "a-k+b"):
        t.context_phone(lab, 0)
    if capi.lib().aasr_device_count() > 0:                     # with one, the step entry simply computes
        t.set_stats(np.array([2.0, 3.0]), np.ones((2, 3)), np.ones((2, 6)))
        sums, _ = t.evaluate([([1, 0], [[1, 1]])])
        assert sums.tolist() == [[5.0] + [2.0] * 9]
        return
    calls = (lambda: t.set_stats(np.ones(2), np.zeros((2, 3)), np.ones((2, 6))), lambda: t.split(), lambda: t.merge(1.0),
             lambda: t.write_model(str(files / "m")))
    for call in calls:
        with pytest.raises(capi.AasrError) as ei:
            call()
        assert ei.value.code == capi.AASR_ERR_NO_DEVICE

"""State tying on the device: the masked-sum and gain kernels through the evaluate entry, trees grown from injected
statistics, and the tool end to end.

Yardsticks: for the sums an exactly rounded sum (math.fsum) with the bound n_members 2^-53 sum |terms|; for the gains
tools/tie_restate.py run with the members in forward, reverse and shuffled order -- the reference sums in the arbitrary
order of a std::set of pointers, so the spread S between orders is its own noise, and the device (a fourth order, a
blocked sum on the matrix pipe) has to stay within 16 S of the forward value; for the trees and the written files the
restatement's decisions, on fixtures whose every decision the restatement itself shows to be 1e-6 clear of a tie or a
threshold."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")
sys.path.insert(0, ROOT)
from aaltoasr_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SPF = 128   # samples per frame at 125 frames a second


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TR = _load("tie_restate")
# Nested phone sets, two of them given twice: two rules that select one member set are skipped as "tried already", and no
# two rules can cut a cluster into the same two halves from opposite sides at one context index -- a set and its
# complement, both "the smaller side" of an even cluster, are one split offered twice, and which of the two equal gains
# wins is decided by rounding in the reference itself.
RULES = "R_ab context a,b\nR_a CONTEXT a\nR_abc context a,b,c\nR_ba context b,a\nR_abcd context a,b,c,d\nR_dcba context d,c,b,a\n"


def pack(m):
    """[n x d x d] symmetric -> [n x d (d + 1) / 2], the lower triangle row-major"""
    il = np.tril_indices(m.shape[1])
    return np.ascontiguousarray(m[:, il[0], il[1]])


def frames_of(rng, d, n, shift=0.0):
    """n frames of a Gaussian whose covariance has condition number <= 100"""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    scale = np.sqrt(np.exp(rng.uniform(0, math.log(100.0), d)))
    return (rng.standard_normal((n, d)) * scale) @ q.T + shift + rng.standard_normal(d)


def stats_of(frames_per_class, d):
    g = np.array([float(len(x)) for x in frames_per_class])
    sx = np.array([x.sum(0) if len(x) else np.zeros(d) for x in frames_per_class])
    sxx = pack(np.array([x.T @ x if len(x) else np.zeros((d, d)) for x in frames_per_class]))
    return g, sx, sxx


@pytest.fixture(scope="module")
def rules_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("tie_rules") / "r.rules"
    p.write_text(RULES)
    return str(p)


_POOLS = {}


def plain_pool(capi, rules_path, d, n_classes, frames_per_class, seed, offset=0.0):
    """a handle with n_classes context phones of one tree and their statistics; shared between the tests of a size"""
    key = (d, n_classes, frames_per_class, seed, offset)
    if key not in _POOLS:
        rng = np.random.default_rng(seed)
        t = capi.Tie(d, rules_path)
        for c in range(n_classes):
            assert t.context_phone("l%d-k+r%d" % (c, c % 7), 0) == c
        frames = [frames_of(rng, d, frames_per_class, offset + 0.3 * (c % 5)) for c in range(n_classes)]
        g, sx, sxx = stats_of(frames, d)
        t.set_stats(g, sx, sxx)
        _POOLS[key] = (t, TR.rows_from_stats(g, sx, sxx))
    return _POOLS[key]


def check_sums(rows, jobs, sums):
    """every value against the exactly rounded sum of its terms, within n_members 2^-53 sum |terms|"""
    at, worst = 0, 0.0
    for members, masks in jobs:
        masks = np.asarray(masks)
        masks = masks.reshape(masks.shape[0], len(members))
        for m in masks:
            sel = [members[k] for k in range(len(members)) if m[k]]
            for e in range(rows.shape[1]):
                terms = [float(rows[c, e]) for c in sel]
                exact = math.fsum(terms)
                bound = len(sel) * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
                err = abs(float(sums[at, e]) - exact)
                assert err <= bound, (at, e, len(sel), err, bound)
                worst = max(worst, err / bound if bound else 0.0)
            at += 1
    assert at == len(sums)
    return worst


def random_job(rng, n_classes, n_members, n_rows):
    members = rng.permutation(n_classes)[:n_members].astype(np.int32)       # not contiguous, not sorted
    masks = (rng.random((n_rows, n_members)) < 0.5).astype(np.uint8)
    return members, masks


@pytest.mark.parametrize("n_members", [1, 3, 4, 5, 63, 64, 65, 130])
def test_masked_sum_member_counts(capi, rules_path, n_members):
    """the K tails of the rank-4 steps and the borders of the 32-bit mask words"""
    t, rows = plain_pool(capi, rules_path, 5, 200, 12, 1)
    rng = np.random.default_rng(100 + n_members)
    job = random_job(rng, 200, n_members, 3)
    job[1][0, :] = 1                                     # the last bit of the last word included
    sums, _ = t.evaluate([job])
    print("worst error / bound:", check_sums(rows, [job], sums))


@pytest.mark.parametrize("n_rows", [1, 15, 16, 17])
def test_masked_sum_rows_per_job(capi, rules_path, n_rows):
    t, rows = plain_pool(capi, rules_path, 5, 200, 12, 1)
    job = random_job(np.random.default_rng(200 + n_rows), 200, 37, n_rows)
    sums, _ = t.evaluate([job])
    assert sums.shape == (n_rows, t.E)
    check_sums(rows, [job], sums)


def test_masked_sum_launch_shape_and_repeatability(capi, rules_path):
    """several jobs of different sizes in one launch, an empty and a full mask among them, a job without members and a
    member listed twice; the same call twice gives the same bytes"""
    t, rows = plain_pool(capi, rules_path, 5, 200, 12, 1)
    rng = np.random.default_rng(7)
    jobs = [random_job(rng, 200, k, r) for k, r in ((130, 17), (1, 1), (33, 2), (64, 16), (5, 40))]
    jobs[0][1][3, :] = 0
    jobs[0][1][4, :] = 1
    jobs[3][1][15, :] = 1
    jobs.append((np.zeros(0, np.int32), np.zeros((2, 0), np.uint8)))
    jobs.append((np.array([9, 9, 4], np.int32), np.array([[1, 1, 0], [0, 1, 1]], np.uint8)))
    cands = [(4, 0, -1), (20 + 15, 20, -1)]             # full masks as parents, a row of the same job as the child
    sums, gain = t.evaluate(jobs, cands)
    check_sums(rows, jobs, sums)
    assert not sums[3].any() and not sums[-4].any() and not sums[-3].any()
    assert t.shape()["items_hop1"] == sum((len(m) + 15) // 16 for _, m in jobs) and t.shape()["items_hop2"] == 0
    sums2, gain2 = t.evaluate(jobs, cands)
    assert sums.tobytes() == sums2.tobytes() and gain.tobytes() == gain2.tobytes()


@pytest.mark.parametrize("d", [1, 5, 15, 39, 63])
def test_masked_sum_dimensions(capi, rules_path, d):
    """E = 3, 21, 136, 820, 2080 values a row against the 16-wide tiles and the work items of four tiles"""
    t, rows = plain_pool(capi, rules_path, d, 40, 8, 2)
    assert t.E == {1: 3, 5: 21, 15: 136, 39: 820, 63: 2080}[d]
    job = random_job(np.random.default_rng(300 + d), 40, 21, 5)
    sums, _ = t.evaluate([job])
    check_sums(rows, [job], sums)
    ep = (t.E + 15) // 16 * 16
    assert t.shape()["items_hop1"] == (ep // 16 + 3) // 4


def restated_gains(rows, d, members, new):
    rest = [m for m in members if m not in new]
    out = []
    for order in ("forward", "reverse", 5):
        out.append(TR.gain(TR.sum_rows(rows, members, order), TR.sum_rows(rows, new, order), TR.sum_rows(rows, rest, order), d))
    return out


@pytest.mark.parametrize("d", [1, 2, 15, 16, 17, 39, 63])
def test_gain_against_the_order_noise_of_the_reference(capi, rules_path, d):
    """40 context phones, a split into 17 and 23 of them; every context phone has d / 4 + 2 frames or more, so every side
    holds at least 4 d.  S = the spread of the restated gain over three member orders; the device within 16 S of the
    forward value, for the other half summed (a row of its own) and for the other half as parent - yes.  The means lie
    three units off the origin, so that the order of the sums shows in the covariance; the gain is a difference of
    products of the size of 10^4, so S comes in steps of their last place, and the split was picked on the CPU (the seed
    600 + d) so that S is not zero at any of the dimensions."""
    per = d // 4 + 2
    assert 17 * per >= 4 * d
    t, rows = plain_pool(capi, rules_path, d, 40, per, 3, offset=3.0)
    rng = np.random.default_rng(600 + d)
    members = [int(c) for c in rng.permutation(40)]
    new = sorted(members[:17])
    members = sorted(members)
    masks = np.array([[1] * 40, [int(m in new) for m in members], [int(m not in new) for m in members]], np.uint8)
    _, gain = t.evaluate([(members, masks)], [(0, 1, 2), (0, 1, -1)], want_sums=False)
    g = restated_gains(rows, d, members, new)
    S = max(g) - min(g)
    print("d %d: gain %.17g  S %.3g  device - forward: summed %.3g, subtracted %.3g" % (d, g[0], S, gain[0] - g[0], gain[1] - g[0]))
    assert S > 0 and all(math.isfinite(x) for x in g)
    assert abs(gain[0] - g[0]) <= 16 * S
    assert abs(gain[1] - g[0]) <= 16 * S


def degenerate_pool(capi, rules_path):
    """one tree of d = 3; the context phone a-k+a has ONE frame: the rule R_a at -1 asks for a side of that one frame,
    whose covariance is exactly zero -- sqrt(0), log(0), 0 / 0.  One right context, so that only the nested sets of the
    left one cut: no split is offered twice."""
    rng = np.random.default_rng(11)
    t = capi.Tie(3, rules_path)
    pool = TR.Pool(TR.read_rules(RULES))
    labels = ["b-k+a", "c-k+a", "a-k+a", "d-k+a", "e-k+a", "f-k+a"]
    frames = []
    for i, lab in enumerate(labels):
        assert t.context_phone(lab, 0) == pool.context_phone(lab, 0) == i
        frames.append(frames_of(rng, 3, 1 if lab == "a-k+a" else 30, 2.0 * (lab[0] in "ab")))
    return t, pool, stats_of(frames, 3)


def test_gain_of_a_degenerate_side_and_what_the_split_does_with_it(capi, rules_path):
    t, pool, (g, sx, sxx) = degenerate_pool(capi, rules_path)
    t.set_stats(g, sx, sxx)
    rows = TR.rows_from_stats(g, sx, sxx)
    members = list(range(6))
    masks = np.array([[1] * 6, [0, 0, 1, 0, 0, 0]], np.uint8)
    _, gain = t.evaluate([(members, masks)], [(0, 1, -1)], want_sums=False)
    want = TR.gain(TR.sum_rows(rows, members), rows[2], TR.sum_rows(rows, [0, 1, 3, 4, 5]), 3)
    assert not math.isfinite(gain[0]) and not math.isfinite(want), (gain[0], want)
    assert math.isnan(gain[0]) == math.isnan(want)
    # --count 1 lets that candidate through; the comparisons skip it as the restatement's do
    r = TR.run(pool, g, sx, sxx, count=1, sgain=0.0, context=1)
    assert any(any(not math.isfinite(x) for x in d["gains"]) for d in r["decisions"])
    assert min(d["lead"] for d in r["decisions"]) >= 1e-6 and min(d["threshold"] for d in r["decisions"]) >= 1e-6
    for hops in (2, 1):
        t.split(count=1, sgain=0.0, context=1, hops=hops)
        assert t.clusters() == r["clusters"], hops
    assert len(r["clusters"]) >= 2


def test_dimension_limit(capi, rules_path):
    with pytest.raises(capi.AasrError) as ei:
        capi.Tie(64, rules_path)
    assert ei.value.code == capi.AASR_ERR_UNSUPPORTED
    capi.Tie(63, rules_path).close()


# ---- trees from injected statistics ------------------------------------------------------------------------------

TREE = dict(seed=9, count=50, sgain=50.0, mloss=50.0)


def tree_fixture(seed):
    """3 centre phones x 3 states, context labels a ... e, d = 5; a fifth of the context phones never seen, one seen
    without frames.  The left context moves the mean of every phone, the right context that of k and s only, and t's
    third state is moved by neither (every context phone still has a random offset of its own)."""
    rng = np.random.default_rng(seed)
    pool = TR.Pool(TR.read_rules(RULES))
    eff_l = {c: 1.2 * rng.standard_normal(5) for c in "abcde"}
    eff_r = {c: 0.8 * rng.standard_normal(5) for c in "abcde"}
    frames, labels = [], []
    for ph in "kst":
        for l in "abcde":
            for r in "abcde":
                if rng.random() < 0.2:
                    continue
                for s in range(3):
                    pool.context_phone("%s-%s+%s" % (l, ph, r), s)
                    labels.append(("%s-%s+%s" % (l, ph, r), s))
                    n = int(rng.integers(8, 40))
                    shift = (0.0 if (ph == "t" and s == 2) else eff_l[l] * (1 + 0.3 * s)) + (eff_r[r] if ph != "t" else 0.0)
                    frames.append(frames_of(rng, 5, n) * 0.5 + shift)
    frames[7] = frames[7][:0]                                   # a context phone whose lines yielded no frames
    return pool, labels, stats_of(frames, 5)


@pytest.fixture(scope="module")
def tree(capi, rules_path):
    pool, labels, (g, sx, sxx) = tree_fixture(TREE["seed"])
    want = TR.run(pool, g, sx, sxx, count=TREE["count"], sgain=TREE["sgain"], context=1)
    want_merged = TR.run(pool, g, sx, sxx, count=TREE["count"], sgain=TREE["sgain"], mloss=TREE["mloss"], context=1)
    return dict(pool=pool, labels=labels, stats=(g, sx, sxx), want=want, merged=want_merged)


def test_tree_fixture_conditions(tree):
    """from the restatement alone: some candidates fail --count, some trees stop early, at least one merge happens and at
    least one does not, two rules select one member set, and every decision is 1e-6 clear"""
    pool, (g, sx, sxx) = tree["pool"], tree["stats"]
    splits = [d for d in tree["merged"]["decisions"] if d["kind"] == "split"]
    merges = [d for d in tree["merged"]["decisions"] if d["kind"] == "merge"]
    assert any(d["win"] is not None for d in splits) and any(d["win"] is None for d in splits)
    assert any(d["win"] is not None for d in merges) and any(d["win"] is None for d in merges)
    sizes = [len(v) for v in tree["want"]["result"].values()]
    assert min(sizes) < max(sizes) and max(sizes) >= 5          # trees of different sizes: --sgain stopped some early
    n_rules = len(pool.rules)
    roots = TR.initial_trees(pool, 1)
    root = roots[0]
    occ = list(g)
    all_c = TR.candidates(pool, occ, root[4], sum(occ[m] for m in root[4]), root[2], root[3], 0)
    kept = TR.candidates(pool, occ, root[4], sum(occ[m] for m in root[4]), root[2], root[3], TREE["count"])
    assert len(kept) < len(all_c) <= 2 * (n_rules - 2)          # --count drops some; R_ba and R_dcba repeat a set
    assert g[7] == 0 and any(7 in c["members"] for c in tree["want"]["clusters"])
    for d in tree["merged"]["decisions"] + tree["want"]["decisions"]:
        assert d["lead"] >= 1e-6 and d["threshold"] >= 1e-6, d


@pytest.mark.parametrize("hops", [2, 1])
def test_trees_equal_the_restatement(capi, rules_path, tree, hops):
    g, sx, sxx = tree["stats"]
    t = capi.Tie(5, rules_path)
    for i, (lab, s) in enumerate(tree["labels"]):
        assert t.context_phone(lab, s) == i
    t.set_stats(g, sx, sxx)
    t.split(count=TREE["count"], sgain=TREE["sgain"], context=1, hops=hops)
    assert t.clusters() == tree["want"]["clusters"]
    assert t.shape()["rounds_split"] >= 3 and (t.shape()["items_hop2"] > 0) == (hops == 2)
    assert t.basebind(1) == TR.basebind_bytes(tree["pool"], tree["want"]["result"], 1)
    t.merge(TREE["mloss"])
    got = t.clusters()
    assert got == tree["merged"]["clusters"]
    assert len(got) < len(tree["want"]["clusters"]) and any(len(c["rules"]) > 1 for c in got)
    assert t.basebind(1) == TR.basebind_bytes(tree["pool"], tree["merged"]["result"], 1)


# ---- the tool end to end -------------------------------------------------------------------------------------------

def write_phn(path, lines):
    with open(path, "w") as f:
        for s, e, lab, k in lines:
            f.write("%d %d %s.%d\n" % (s * SPF, e * SPF, lab, k))


def collect(pool, utts):
    """collect_phone_stats: per line the frames start ... end - 1; the feature end cuts the line and the file"""
    per_class = {}
    for frames, lines in utts:
        for s, e, lab, k in lines:
            c = pool.context_phone(lab, k)
            per_class.setdefault(c, [])
            per_class[c].append(frames[s:min(e, len(frames))])
            if e > len(frames):
                break
    d = utts[0][0].shape[1]
    return [np.concatenate(per_class[c]) if per_class[c] else np.zeros((0, d)) for c in range(len(pool.classes))]


def read_gk_full(path):
    toks = open(path).read().split()
    n, d = int(toks[0]), int(toks[1])
    assert toks[2] == "variable"
    vals = np.array([float(x) for x in toks[3:] if x != "full"]).reshape(n, d + d * d)
    assert toks[3::1 + d + d * d] == ["full"] * n
    return vals[:, :d], vals[:, d:].reshape(n, d, d)


def check_gk(path, per_class, clusters, want_gk_text, tmp):
    """entry by entry within n_frames 2^-52 (sum |x_i x_j| / gamma + |mu_i mu_j|) of the restatement's own text; the means
    within n_frames 2^-52 sum |x_i| / gamma"""
    open(tmp, "w").write(want_gk_text)
    mu, cov = read_gk_full(path)
    want_mu, want_cov = read_gk_full(tmp)
    assert mu.shape == want_mu.shape
    for s, cl in enumerate(clusters):
        x = np.concatenate([per_class[c] for c in cl["members"]])
        n = len(x)
        bound = n * 2.0 ** -52 * (np.abs(x).T @ np.abs(x) / n + np.abs(np.outer(want_mu[s], want_mu[s])))
        assert np.all(np.abs(cov[s] - want_cov[s]) <= bound), s
        assert np.all(np.abs(mu[s] - want_mu[s]) <= n * 2.0 ** -52 * np.abs(x).sum(0) / n), s


TOOL = dict(seed=0, count=60, sgain=20.0, mloss=30.0)
# no two of these rules can halve a cluster into the same two parts: a split that two candidates offer (a set and its
# complement, both "the smaller side" of an even cluster) is a tie that the reference itself decides by rounding
TOOL_RULES = "A context a\nAB context a,b\nD context d\n"


def tool_utterances(seed):
    """two utterances of a pre module's frames, d = 4: centre phones k and s and the silence _ in contexts a, b, c; the
    second utterance's .phn runs past its features: the line across the end is cut, the lines after it are never read"""
    rng = np.random.default_rng(seed)
    eff = {c: 1.5 * rng.standard_normal(4) for c in "abc"}
    utts = []
    for u in range(2):
        frames, lines, at = [], [], 0
        for rep in range(70):
            ph = "ks"[int(rng.integers(0, 2))]
            l, r = "abc"[int(rng.integers(0, 3))], "abc"[int(rng.integers(0, 3))]
            for k in range(2):
                n = int(rng.integers(3, 9))
                frames.append(frames_of(rng, 4, n) * 0.4 + eff[l] * (1 + k) + (0.7 * eff[r] if ph == "k" else 0.0))
                lines.append((at, at + n, "%s-%s+%s" % (l, ph, r), k))
                at += n
            if rep % 10 == 9:
                n = int(rng.integers(3, 9))
                frames.append(frames_of(rng, 4, n) * 0.2)
                lines.append((at, at + n, "_", 0))
                at += n
        x = np.concatenate(frames).astype(np.float32)
        if u == 0:
            lines.insert(40, (lines[40][0], lines[40][0], "d-s+a", 1))   # an empty line: its context phone still exists
        if u == 1:
            cut = lines[-3][0] + 2                               # in the middle of the third line from the end
            x = x[:cut]
            lines[-1] = (lines[-1][0], lines[-1][1], "e-k+e", 0)  # after the cut: never read, it does not exist
        utts.append((x, lines))
    return utts


@pytest.fixture(scope="module")
def tool(capi, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("tie_tool")
    utts = tool_utterances(TOOL["seed"])
    open(str(d / "k.cfg"), "w").write("module\n{\n name pre\n type pre\n dim 4\n}\n")
    rules = TOOL_RULES
    open(str(d / "k.rules"), "w").write(rules)
    recipe = []
    for u, (x, lines) in enumerate(utts):
        oracle.write_feature_file(str(d / ("u%d.fea" % u)), x)
        write_phn(str(d / ("u%d.phn" % u)), lines)
        recipe.append("audio=%s transcript=%s" % (d / ("u%d.fea" % u), d / ("u%d.phn" % u)))
    open(str(d / "k.rcp"), "w").write("\n".join(recipe) + "\n")
    pool = TR.Pool(TR.read_rules(rules))
    per_class = collect(pool, [(x.astype(np.float64), lines) for x, lines in utts])
    g, sx, sxx = stats_of(per_class, 4)
    return dict(dir=d, pool=pool, per_class=per_class, stats=(g, sx, sxx))


def run_tie(tool, *args):
    d = tool["dir"]
    cmd = [os.path.join(BIN, "tie"), "-c", str(d / "k.cfg"), "-r", str(d / "k.rcp"), "-u", str(d / "k.rules"),
           "--count", str(TOOL["count"]), "--sgain", str(TOOL["sgain"])] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


def test_tool_fixture_conditions(tool):
    g = tool["stats"][0]
    keys = [(c[0], c[1]) for c in tool["pool"].classes]
    assert ("_", 0) in keys and g[keys.index(("d-s+a", 1))] == 0 and ("e-k+e", 0) not in keys
    for mloss in (None, TOOL["mloss"]):
        r = TR.run(tool["pool"], *tool["stats"], count=TOOL["count"], sgain=TOOL["sgain"], mloss=mloss, context=1)
        assert len(r["clusters"]) > len(tool["pool"].phones) + 2
        for d in r["decisions"]:
            assert d["lead"] >= 1e-6 and d["threshold"] >= 1e-6, d


def test_tool_basebind_is_the_restatement_byte_for_byte(capi, tool):
    out = str(tool["dir"] / "o.basebind")
    run_tie(tool, "-B", out)
    r = TR.run(tool["pool"], *tool["stats"], count=TOOL["count"], sgain=TOOL["sgain"], context=1)
    want = TR.basebind_bytes(tool["pool"], r["result"], 1)
    assert open(out, "rb").read() == want
    assert want.startswith(b"_ 1 0\na-k+a 2 ")
    out_m = str(tool["dir"] / "m.basebind")
    run_tie(tool, "-B", out_m, "--mloss", TOOL["mloss"])
    rm = TR.run(tool["pool"], *tool["stats"], count=TOOL["count"], sgain=TOOL["sgain"], mloss=TOOL["mloss"], context=1)
    assert open(out_m, "rb").read() == TR.basebind_bytes(tool["pool"], rm["result"], 1)
    assert len(rm["clusters"]) < len(r["clusters"])


def test_tool_model_files_load_and_score(capi, tool):
    base = str(tool["dir"] / "o")
    run_tie(tool, "-o", base)
    r = TR.run(tool["pool"], *tool["stats"], count=TOOL["count"], sgain=TOOL["sgain"], context=1)
    mc, ph, gk, mu, cov = TR.model_texts(tool["pool"], r["result"], 1, r["rows"], 4)
    assert open(base + ".mc").read() == mc and open(base + ".ph").read() == ph
    check_gk(base + ".gk", tool["per_class"], r["clusters"], gk, str(tool["dir"] / "want.gk"))
    gmm = capi.Gmm.from_files(base + ".gk", base + ".mc", base + ".ph")
    assert gmm.num_states == len(r["clusters"]) and gmm.dim == 4
    got_mu, got_cov = read_gk_full(base + ".gk")
    x = np.concatenate([tool["per_class"][c] for c in r["clusters"][1]["members"]])[:16]
    score = gmm.score(x.astype(np.float32)).astype(np.float64)      # the float32 scoring of a full-covariance pool
    want = np.empty_like(score)
    for s in range(len(got_mu)):
        diff = x - got_mu[s]
        # FullCovarianceGaussian's constant is log sqrt det P alone, without the (2 pi)^(d / 2)
        want[:, s] = -0.5 * (np.einsum("fi,ij,fj->f", diff, np.linalg.inv(got_cov[s]), diff) + np.linalg.slogdet(got_cov[s])[1])
    print("largest score difference:", np.abs(score - want).max())
    assert np.all(np.isfinite(score)) and np.allclose(score, np.maximum(want, math.log(1e-50)), rtol=1e-3, atol=1e-2)


VTLN_CFG = """module
{
  name audiofile
  type audiofile
  sample_rate 16000
}
module
{
  name fft
  type fft
  magnitude 0
  sources audiofile
}
module
{
  name vtln
  type vtln
  sources fft
}
module
{
  name mel
  type mel
  sources vtln
}
module
{
  name mfcc
  type dct
  dim 6
  sources mel
}
"""
SPKC = "speaker s1\n{\n  feature vtln\n  {\n    warp_factor 0.92\n  }\n}\nspeaker s2\n{\n  feature vtln\n  {\n    warp_factor 1.08\n  }\n}\n"


def test_tool_speaker_file_changes_the_statistics(capi, oracle, tmp_path):
    """-S: every utterance's features under its speaker's VTLN warp.  --count is out of reach, so every tree stays its
    root and the model's Gaussians are the phones' statistics themselves."""
    import wave
    d = tmp_path
    open(str(d / "v.cfg"), "w").write(VTLN_CFG)
    open(str(d / "v.spkc"), "w").write(SPKC)
    open(str(d / "v.rules"), "w").write("A context a\n")
    ft = capi.Feat(VTLN_CFG)
    recipe, utts = [], {"warped": [], "flat": []}
    for u, (sp, warp) in enumerate((("s1", "0.92"), ("s2", "1.08"))):
        pcm = synth.make_audio(16000, seed=60 + u)
        with wave.open(str(d / ("u%d.wav" % u)), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.asarray(pcm, np.int16).tobytes())
        eof = ft.eof_frame(len(pcm))
        lines = [(f, min(f + 10, eof), "%s-k+%s" % ("ab"[(f // 10) % 2], "ab"[(f // 20) % 2]), (f // 10) % 2)
                 for f in range(0, eof, 10)]
        write_phn(str(d / ("u%d.phn" % u)), lines)
        recipe.append("audio=%s transcript=%s speaker=%s" % (d / ("u%d.wav" % u), d / ("u%d.phn" % u), sp))
        for name, wf in (("warped", warp), ("flat", "1.0")):
            ft.set_parameters("vtln", "{\n  warp_factor %s\n}\n" % wf)
            utts[name].append((ft.run(pcm, 0, eof, dtype=np.float64), lines))
    open(str(d / "v.rcp"), "w").write("\n".join(recipe) + "\n")
    base = str(d / "o")
    r = subprocess.run([os.path.join(BIN, "tie"), "-c", str(d / "v.cfg"), "-r", str(d / "v.rcp"), "-u", str(d / "v.rules"),
                        "-S", str(d / "v.spkc"), "--count", "100000", "-o", base], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = {}
    for name in utts:
        pool = TR.Pool(TR.read_rules("A context a\n"))
        per_class = collect(pool, utts[name])
        run = TR.run(pool, *stats_of(per_class, ft.dim), count=100000, context=1)
        res[name] = (per_class, run, TR.model_texts(pool, run["result"], 1, run["rows"], ft.dim))
    per_class, run, (mc, ph, _gk, mu, cov) = res["warped"]
    assert open(base + ".mc").read() == mc and open(base + ".ph").read() == ph and len(run["clusters"]) == 2
    check_gk(base + ".gk", per_class, run["clusters"], _gk, str(d / "want.gk"))
    got_mu, _ = read_gk_full(base + ".gk")
    assert np.abs(got_mu - res["flat"][2][3]).max() > 1e-3 * np.abs(got_mu).max()      # the warps matter

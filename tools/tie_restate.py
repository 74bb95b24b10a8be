"""aku/tie.cc over aku/PhonePool.cc restated in NumPy float64: the yardstick of tests/test_tie_host.py and
tests/test_tie_gpu.py, and the CPU baseline of tools/bench_tie.py.

What is restated: the label functions, the rule file, the context phones in the pool's ordered containers, the
candidates of apply_best_splitting_rule (the --count test, the smaller side, the skip of a member set already tried), the
split loop with its `c--` (the cluster order is the state numbering), the greedy merge, the basebind writer and
save_model's three text files.

Arithmetic: a cluster's statistic is the sum of its members' raw rows [gamma, sum x, packed lower triangle of
sum x x^T] -- what Gaussian::merge rebuilds from occ (Sigma + mu mu^T) -- added one member at a time in the ORDER GIVEN
(`order`: "forward", "reverse" or a seed for a shuffle; the reference walks a std::set of pointers, so its order is
arbitrary and the spread between orders is its own noise).  mu = sum x / gamma, Sigma = sum x x^T / gamma - mu mu^T,
LinearAlgebra::cholesky_factor column by column with its subtractions in k order, log det = 2 sum log L_ii,
gain = (gamma_p ld_p - gamma_1 ld_1 - gamma_2 ld_2) / 2.  NumPy's elementwise operations are correctly rounded and never
fused.  A matrix that is not positive definite gives NaN or an infinity, as IEEE arithmetic does, and the comparisons
(`gain > best and gain > sgain`, `gain < min_loss`) then do what they do.

Every decision is recorded with its margin: the relative lead of the winner over the best other candidate and the
relative distance of every compared gain from its threshold.  A kernel that rounds differently can change a decision only
where such a margin is at rounding level.
"""
import math

import numpy as np


# ---- labels ---------------------------------------------------------------------------------------

def center_phone(label):
    pos1, pos2 = label.rfind("-"), label.find("+")
    temp = ""
    if pos1 >= 0 and pos2 >= 0:
        if pos2 > pos1 + 1:
            temp = label[pos1 + 1:pos2]
    elif pos1 >= 0:
        temp = label[pos1 + 1:]
    elif pos2 >= 0:
        temp = label[:pos2]
    else:
        temp = label
    if not temp:
        raise ValueError("PhonePool: Invalid phone label" + label)
    return temp


def left_contexts(label):
    """nearest first"""
    out, cur = [], 0
    while True:
        nxt = label.find("-", cur + 1)
        if nxt < cur:
            break
        out.append(label[cur:nxt])
        cur = nxt + 1
    return out[::-1]


def right_contexts(label):
    out, cur = [], label.find("+")
    if cur > 0:
        cur += 1
        while True:
            nxt = label.find("+", cur + 1)
            if nxt < cur:
                break
            out.append(label[cur:nxt])
            cur = nxt + 1
        out.append(label[cur:])
    return out


def read_rules(text):
    """-> [(name, frozenset of phones)]; the reference's errors as ValueError"""
    rules = []
    for line in text.split("\n"):
        line = line.strip(" \t\r")
        if not line:
            continue
        fields = line.replace("\t", " ").split(None, 2)
        if len(fields) < 2:
            raise ValueError("PhonePool::load_decision_tree_rules: Invalid rule line:\n" + line)
        if fields[1].lower() != "context":
            raise ValueError("PhonePool::load_decision_tree_rules: Invalid rule type " + fields[1].lower())
        phones = [p for p in fields[2].replace(",", " ").split()] if len(fields) > 2 else []
        if not phones:
            raise ValueError("PhonePool::load_decision_tree_rules: No phones in the context rule:\n" + line)
        rules.append((fields[0], frozenset(phones)))
    return rules


class Pool:
    """The context phones: class index = order of first mention; phones, per-state maps and contexts are ordered."""

    def __init__(self, rules):
        self.rules = rules
        self.phones = {}          # centre -> [ {label: class} per state ]
        self.contexts = set()
        self.classes = []         # (label, state, left, right)

    def context_phone(self, label, state):
        states = self.phones.setdefault(center_phone(label), [])
        while len(states) <= state:
            states.append({})
        if label not in states[state]:
            l, r = left_contexts(label), right_contexts(label)
            self.contexts.update(l + r)
            states[state][label] = len(self.classes)
            self.classes.append((label, state, l, r))
        return states[state][label]

    def answer(self, contexts, rule, ci):
        left, right = contexts
        if ci < 0:
            return -ci <= len(left) and left[-ci - 1] in self.rules[rule][1]
        return ci <= len(right) and right[ci - 1] in self.rules[rule][1]


def _bytes_sorted(keys):
    return sorted(keys, key=lambda s: s.encode("latin-1"))   # std::string compares bytes


# ---- statistics -----------------------------------------------------------------------------------

def rows_from_stats(gamma, sum_x, sum_xx):
    return np.concatenate([np.asarray(gamma, np.float64)[:, None], np.asarray(sum_x, np.float64),
                           np.asarray(sum_xx, np.float64)], axis=1)


def ordered(members, order):
    m = list(members)
    if order == "forward":
        return m
    if order == "reverse":
        return m[::-1]
    rng = np.random.default_rng(order)
    return [m[i] for i in rng.permutation(len(m))]


def sum_rows(rows, members, order="forward"):
    acc = np.zeros(rows.shape[1])
    for m in ordered(members, order):
        acc = acc + rows[m]
    return acc


def mean_cov(row, d):
    with np.errstate(all="ignore"):
        gamma = row[0]
        mu = row[1:1 + d] / gamma
        cov = np.zeros((d, d))
        il = np.tril_indices(d)
        cov[il] = row[1 + d:] / gamma - mu[il[0]] * mu[il[1]]
        cov = cov + np.tril(cov, -1).T
    return mu, cov


def _log(x):
    if x > 0:
        return math.log(x) if x != math.inf else math.inf
    return -math.inf if x == 0 else math.nan


def log_det(cov):
    """2 sum log L_ii of the reference's column Cholesky, no pivot test"""
    d = cov.shape[0]
    B = np.array(cov, np.float64)
    with np.errstate(all="ignore"):
        for j in range(d):
            col = B[j:, j].copy()
            for k in range(j):
                col = col - B[j:, k] * B[j, k]
            ljj = np.sqrt(col[0])
            B[j, j] = ljj
            B[j + 1:, j] = col[1:] / ljj
    s = 0.0
    for i in range(d):
        s = s + _log(float(B[i, i]))
    return s * 2


def gain(parent, child1, child2, d):
    with np.errstate(all="ignore"):
        lp, l1, l2 = (log_det(mean_cov(r, d)[1]) for r in (parent, child1, child2))
        return float((np.float64(lp) * parent[0] - np.float64(l1) * child1[0] - np.float64(l2) * child2[0]) / 2)


def _rel(a, b):
    """relative distance of a from b in units of |a|; inf when either is not finite"""
    if not (math.isfinite(a) and math.isfinite(b)):
        return math.inf
    return abs(a - b) / abs(a) if a != 0 else (math.inf if b != 0 else 0.0)


# ---- the trees ------------------------------------------------------------------------------------

def initial_trees(pool, context):
    """-> [(phone, state, ctx_start, ctx_end, [cluster])] in pool order; cluster = {"members", "rules", "occ"}"""
    trees = []
    for ph in _bytes_sorted(pool.phones):
        states = pool.phones[ph]
        ml = max([len(pool.classes[c][2]) for st in states for c in st.values()] + [0])
        mr = max([len(pool.classes[c][3]) for st in states for c in st.values()] + [0])
        for s, st in enumerate(states):
            lo, hi = (-min(ml, context), min(mr, context)) if context > 0 else (-ml, mr)
            trees.append((ph, s, lo, hi, sorted(st.values())))
    return trees


def candidates(pool, occ, members, cl_occ, lo, hi, count):
    """apply_best_splitting_rule's candidates that reach the gain, in its order: (rule, context, first_answer, set)"""
    out, seen = [], []
    for r in range(len(pool.rules)):
        for i in range(lo, hi + 1):
            if i == 0:
                continue
            ans = [pool.answer(pool.classes[m][2:4], r, i) for m in members]
            c1 = sum(occ[m] for m, a in zip(members, ans) if a)
            c2 = cl_occ - c1
            if c1 < count or c2 < count:
                continue
            first = sum(ans) <= len(members) // 2
            new = [m for m, a in zip(members, ans) if a == first]
            if new in seen:
                continue
            seen.append(new)
            out.append((r, i, first, new))
    return out


def split(pool, occ, count, sgain, context, gain_of, decisions=None):
    """decision_tree_cluster_context_phones with gain_of(members, new_set) -> gain.  -> {(phone, state): [cluster]}"""
    result = {}
    for ph, s, lo, hi, members in initial_trees(pool, context):
        clusters = [{"members": members, "rules": [[]], "occ": sum(occ[m] for m in members)}]
        c = 0
        while c < len(clusters):
            cl = clusters[c]
            cands = candidates(pool, occ, cl["members"], cl["occ"], lo, hi, count)
            gains = [gain_of(cl["members"], new) for (_r, _i, _f, new) in cands]
            best, win = -1.0, None
            for k, g in enumerate(gains):
                if g > best and g > sgain:
                    best, win = g, k
            if decisions is not None and cands:
                finite = [g for g in gains if not math.isnan(g)]
                top = max(finite) if finite else math.nan
                others = [g for k, g in enumerate(gains) if k != win and not math.isnan(g)]
                decisions.append({"kind": "split", "phone": ph, "state": s, "gains": gains, "win": win,
                                  "lead": _rel(best, max(others)) if win is not None and others else math.inf,
                                  "threshold": min([_rel(g, sgain) for g in finite] + [_rel(top, -1.0) if finite else math.inf])})
            if win is None:
                c += 1
                continue
            r, i, first, new = cands[win]
            rest = [m for m in cl["members"] if m not in new]
            other = {"members": rest, "rules": [cl["rules"][0] + [(r, i, not first)]], "occ": sum(occ[m] for m in rest)}
            cl["members"], cl["occ"] = new, sum(occ[m] for m in new)
            cl["rules"] = [cl["rules"][0] + [(r, i, first)]]
            clusters.append(other)
        result[(ph, s)] = clusters
    return result


def merge(result, mloss, pair_gain, decisions=None):
    """merge_context_phones with pair_gain(members_c, members_i) -> gain, in place"""
    for key, clusters in result.items():
        c = 0
        while c < len(clusters):
            min_loss, target, gains = 2 * mloss, -1, []
            for i in range(c + 1, len(clusters)):
                g = pair_gain(clusters[c]["members"], clusters[i]["members"])
                gains.append(g)
                if g < min_loss:
                    min_loss, target = g, i
            if decisions is not None and gains:
                finite = sorted(g for g in gains if not math.isnan(g))
                decisions.append({"kind": "merge", "phone": key[0], "state": key[1], "gains": gains,
                                  "win": target if min_loss < mloss else None,
                                  "lead": _rel(finite[0], finite[1]) if len(finite) > 1 else math.inf,
                                  "threshold": min(_rel(finite[0], mloss), _rel(finite[0], 2 * mloss)) if finite else math.inf})
            if min_loss < mloss and target > c:
                a, o = clusters[c], clusters[target]
                a["rules"] = a["rules"] + o["rules"]
                a["members"] = sorted(set(a["members"]) | set(o["members"]))
                a["occ"] = a["occ"] + o["occ"]
                del clusters[target]
            else:
                c += 1
    return result


def final_clusters(pool, result):
    """-> the clusters in state order: [{"phone", "state", "index", "occ", "members", "rules"}], rules by name"""
    out = []
    for ph in _bytes_sorted(pool.phones):
        for s in range(len(pool.phones[ph])):
            for cl in result[(ph, s)]:
                rules = [] if cl["rules"] == [[]] else [[(pool.rules[r][0], i, bool(a)) for (r, i, a) in rs] for rs in cl["rules"]]
                out.append({"phone": ph, "state": s, "index": len(out), "occ": float(cl["occ"]),
                            "members": list(cl["members"]), "rules": rules})
    return out


# ---- the writers ----------------------------------------------------------------------------------

def hmms(pool, result, context):
    """iterate_context_phones: [(label, [state index per HMM state])]"""
    index, n = {}, 0
    for ph in _bytes_sorted(pool.phones):
        for s in range(len(pool.phones[ph])):
            for k in range(len(result[(ph, s)])):
                index[(ph, s, k)] = n
                n += 1
    ctx = _bytes_sorted(pool.contexts)
    out = []
    for ph in _bytes_sorted(pool.phones):
        ns = len(pool.phones[ph])
        if ph[0] == "_" or context <= 0:
            out.append((ph, [index[(ph, s, 0)] for s in range(ns)]))
            continue
        if not ctx:
            continue
        it = [0] * (2 * context)
        while True:
            label = "".join(ctx[it[i]] + "-" for i in range(context)) + ph + "".join("+" + ctx[it[i]] for i in range(context, 2 * context))
            lr = (left_contexts(label), right_contexts(label))
            states = []
            for s in range(ns):
                cls = result[(ph, s)]
                found = 0 if len(cls) == 1 else -1
                for k, cl in enumerate(cls):
                    if found >= 0:
                        break
                    for rs in cl["rules"]:
                        if all(pool.answer(lr, r, i) == a for (r, i, a) in rs):
                            found = k
                            break
                if found < 0:
                    raise ValueError("no cluster takes " + label)
                states.append(index[(ph, s, found)])
            out.append((label, states))
            i = 2 * context - 1
            while i >= 0:
                it[i] += 1
                if it[i] != len(ctx):
                    break
                if i > 0:
                    it[i] = 0
                i -= 1
            if it[0] == len(ctx):
                break
    return out


def basebind_bytes(pool, result, context):
    return "".join("%s %d%s\n" % (label, len(st), "".join(" %d" % s for s in st)) for label, st in hmms(pool, result, context)
                   ).encode("latin-1")


def model_texts(pool, result, context, rows, d, order="forward"):
    """save_model: -> (mc text, ph text, gk text, means [S x d], covariances [S x d x d])"""
    cls = final_clusters(pool, result)
    mc = "%d\n" % len(cls) + "".join("1 %d 1\n" % s for s in range(len(cls)))
    hs = hmms(pool, result, context)
    ph = "PHONE\n%d\n" % len(hs)
    for h, (label, st) in enumerate(hs):
        ph += "%d %d %s\n-1 -2%s\n0 1 2 1\n1 0\n" % (h + 1, len(st) + 2, label, "".join(" %d" % s for s in st))
        for s in range(len(st)):
            ph += "%d 2 %d 0.8 %d 0.2\n" % (s + 2, s + 2, 1 if s + 3 == len(st) + 2 else s + 3)
    means, covs = np.zeros((len(cls), d)), np.zeros((len(cls), d, d))
    gk = "%d %d variable\n" % (len(cls), d)
    for s, cl in enumerate(cls):
        means[s], covs[s] = mean_cov(sum_rows(rows, cl["members"], order), d)
        gk += "full " + "".join("%g " % v for v in means[s]) + " ".join("%g" % v for v in covs[s].reshape(-1)) + "\n"
    return mc, ph, gk, means, covs


def run(pool, gamma, sum_x, sum_xx, count=100, sgain=0.0, mloss=None, context=1, order="forward"):
    """The whole search on given statistics -> {"clusters", "decisions", "result", "rows"}"""
    rows = rows_from_stats(gamma, sum_x, sum_xx)
    d = np.asarray(sum_x).shape[1]
    occ = [float(g) for g in gamma]
    decisions = []

    def split_gain(members, new):
        parent = sum_rows(rows, members, order)
        c1 = sum_rows(rows, new, order)
        c2 = sum_rows(rows, [m for m in members if m not in new], order)
        return gain(parent, c1, c2, d)

    def pair_gain(a, b):
        ra, rb = sum_rows(rows, a, order), sum_rows(rows, b, order)
        return gain(ra + rb, ra, rb, d)

    result = split(pool, occ, count, sgain, context, split_gain, decisions)
    if mloss is not None:
        merge(result, mloss, pair_gain, decisions)
    return {"clusters": final_clusters(pool, result), "decisions": decisions, "result": result, "rows": rows}

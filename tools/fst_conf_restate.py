"""fst_conf_restate.py -- the FST decoder's confidence (csrc/fst_conf.hip, csrc/fst_conf.cc) restated in NumPy float32 on
top of fst_restate.py: the yardstick of its tests.

It follows the reference's decoder/src/FstConfidence.{hh,cc} operation by operation, every float32 operation rounded on
its own: the frame-best sum (start -999999999.9f, replaced on strict >, summed in frame order), both run() variants (the
plain FstConfidence discards the frame maximum: its best_acu_score stays 0), the best different hypothesis among
Result.tokens, remove_junk and the byte edit distance, and the five formulas with std::min / std::max operand order
(std::min(a, b) is b when b < a, else a; std::max(a, b) is b when a < b, else a -- a NaN second operand never wins).
Where the reference is undefined: without an end-node token best_final_logprob is -9999999.9f, token_conf -9999999.9f and
no_final is set; zero frames keep the IEEE result of the division.  Ties that could change an output are those
fst_restate.search reports for either search; nothing here hides one.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fst_restate as R  # noqa: E402

F32 = np.float32
NONE = F32(-9999999.9)
ACU_START = F32(-999999999.9)
FLOATS = ("confidence", "token_conf", "ploop_conf", "edit_conf", "best_acu_conf", "grammar_logprob", "ploop_logprob",
          "best_final_logprob", "best_different_logprob", "best_acu_score")


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def frame_best(ac: np.ndarray) -> np.ndarray:
    """get_best_frame_acu_prob of every frame: float32 [frames]"""
    out = np.zeros(ac.shape[0], np.float32)
    for t in range(ac.shape[0]):
        best = ACU_START
        for x in ac[t]:
            if x > best:
                best = x
        out[t] = best
    return out


def frame_best_sum(ac: np.ndarray) -> np.float32:
    s = F32(0)
    with np.errstate(all="ignore"):
        for x in frame_best(ac):
            s = F32(s + x)
    return s


def best_different(tokens, end):
    """tokens: Result.tokens (descending); end: node_end.  -> (has_final, words of the best end-node token, its
    log-probability or NONE, the log-probability of the first token whose words differ or NONE, whether there is one)"""
    final = next((tk for tk in tokens if end[tk[0]]), None)
    if final is None:
        return False, (), NONE, NONE, False
    other = next((tk for tk in tokens if tk[3] != final[3]), None)
    return True, final[3], F32(final[1]), (F32(other[1]) if other is not None else NONE), other is not None


def remove_junk(s: bytes) -> bytes:
    out, prev = bytearray(), 0x20
    for c in s:
        if c == 0x20 or c == prev:
            continue
        prev = c
        out.append(c)
    return bytes(out)


def edit_distance(a: bytes, b: bytes) -> int:
    prev = list(range(len(b) + 1))
    for i in range(len(a)):
        cur = [i + 1]
        for j in range(len(b)):
            cur.append(min(cur[j] + 1, prev[j + 1] + 1, prev[j] + (a[i] != b[j])))
        prev = cur
    return prev[len(b)]


def formulas(frames: int, grammar_lp, ploop_lp, best_final_lp, best_different_lp, best_acu_score, n_words: int, grammar: bytes,
             ploop) -> dict:
    """ploop None: the plain FstConfidence (0.5 * (token + best_acu), the product in double, stored to float)"""
    f = F32(frames)
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        r = {"grammar_logprob": F32(grammar_lp), "ploop_logprob": F32(ploop_lp), "best_final_logprob": F32(best_final_lp),
             "best_different_logprob": F32(best_different_lp), "best_acu_score": F32(best_acu_score)}
        r["best_acu_conf"] = F32(F32(1.5) - F32(F32(F32(0.25) * F32(F32(-best_final_lp) + best_acu_score)) / f))
        if n_words == 0:
            r["token_conf"] = NONE
        else:
            x = F32(F32(0.2) - F32(F32(F32(5) * F32(F32(-best_final_lp) + best_different_lp)) / f))
            r["token_conf"] = std_max(zero, std_min(one, x))
        if ploop is None:
            r["ploop_conf"] = r["edit_conf"] = zero
            r["confidence"] = F32(0.5 * float(F32(r["token_conf"] + r["best_acu_conf"])))
            return r
        r["ploop_conf"] = std_min(one, F32(one - F32(F32(F32(0.25) * F32(F32(-grammar_lp) + ploop_lp)) / f)))
        cg, cp = remove_junk(grammar), remove_junk(ploop)
        r["edit_conf"] = std_max(zero, F32(one - F32(F32(edit_distance(cg, cp)) / F32(len(cg)))))
        total = F32(std_min(one, r["ploop_conf"]) + F32(F32(20) * std_min(one, r["token_conf"])))
        total = F32(total + F32(F32(5) * std_min(one, r["edit_conf"])))
        total = F32(total + std_min(one, r["best_acu_conf"]))
        r["confidence"] = F32(total / F32(27))
    return r


class Conf:
    """grammar, phone: fst_restate.Result (phone None: plain); r: the ten floats; text, ploop_text; no_final; ties"""


def confidence(net, ac, gopt: dict, durations=None, phone_net=None, popt: dict = None) -> Conf:
    """gopt / popt: beam, token_limit, duration_scale, transition_scale of the two searches (popt None: FstSearch's
    defaults).  phone_net None: the reference's plain FstConfidence."""
    c = Conf()
    c.grammar = R.search(net, ac, durations=durations, **gopt)
    c.phone = R.search(phone_net, ac, durations=durations, **(popt or {})) if phone_net is not None else None
    c.ties = list(c.grammar.ties) + (list(c.phone.ties) if c.phone is not None else [])
    c.text = c.grammar.text(net.symbols)
    c.ploop_text = c.phone.text(phone_net.symbols) if c.phone is not None else None
    has_final, words, bf, bd, c.has_different = best_different(c.grammar.tokens, net.node_end)
    c.no_final = not has_final
    c.n_words = len(words)
    acu = frame_best_sum(ac) if c.phone is not None else F32(0)
    c.r = formulas(ac.shape[0], c.grammar.logprob, c.phone.logprob if c.phone is not None else F32(-1), bf, bd, acu,
                   len(words) if has_final else 0, c.text, c.ploop_text)
    return c


def random_phone_loop(rng, n_models: int, n_phones: int = 6, states: int = 2, letters: bytes = b"abcdefghijklmnopqrstuvwxyz") -> bytes:
    """A random phone-loop network in the file's text form: node 0 is the loop's hub (initial, end, non-emitting); every
    phone is a chain of emitting states with self-loops, its single-letter symbol (letters, in turn) on the arc that
    leaves the hub; a phone's last state is an end node too and leads back to the hub."""
    lines, node = [b"I 0"], 1
    for ph in range(n_phones):
        pdfs = [int(rng.integers(0, n_models)) for _ in range(states)]
        for k, pdf in enumerate(pdfs):
            src = 0 if k == 0 else node - 1
            sym = letters[ph % len(letters):ph % len(letters) + 1] if k == 0 else b","
            lines.append(b"T %d %d %d %s %.6f" % (src, node, pdf, sym, -float(rng.random()) * 2))
            lines.append(b"T %d %d %d , %.6f" % (node, node, pdf, -float(rng.random())))
            node += 1
        lines.append(b"T %d 0 -1 , %.6f" % (node - 1, -float(rng.random())))
        lines.append(b"F %d" % (node - 1))
    lines.append(b"F 0")
    return R.write_fst(lines)

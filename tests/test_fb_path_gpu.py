"""The best path out of the forward-backward kernel (aasr_fb_options.want_path, aasr_fb_batch_path; csrc/hmmnet_fb.hip)
against tools/hmmnet_restate.py's Viterbi path, arc for arc.  The inputs are tools/align_restate.py::path_cases;
tests/test_stats_align_host.py holds every one of them to a lead of 1e-6 over the runner-up, so no rounding decides a path
and the comparison is exact.  Both forms of the kernel (LDS and force_global), float and double rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import align_restate as AR  # noqa: E402
import hmmnet_cases as HC  # noqa: E402

RS = HC.RS
pytestmark = pytest.mark.gpu
S = 40
WIDE = 1e9
CASES = AR.path_cases()
IDS = ["%s-%d" % (c[0], c[2]) for c in CASES]


@pytest.fixture(scope="module")
def model(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("fb_path")
    sp = HC.self_probs(S)
    HC.write_ph(str(d / "m.ph"), sp)
    return {"dir": d, "sp": sp, "topo": capi.Topology(str(d / "m.ph")), "n": [0]}


def _net(capi, model, text):
    model["n"][0] += 1
    p = str(model["dir"] / ("n%d.hmmnet" % model["n"][0]))
    open(p, "w").write(text)
    return capi.HmmNet(model["topo"], p), HC.parse(text, model["sp"])


def _run(capi, nets, lls, want_path=True, force_global=False, bw=WIDE, max_attempts=1):
    import torch
    o = capi.FbOptions.defaults()
    o.fw_beam, o.bw_beam = WIDE, bw
    o.mode = capi.FB_VITERBI
    o.want_pdf_occ = o.want_tr_occ = 1
    o.want_path = 1 if want_path else 0
    o.force_global = 1 if force_global else 0
    o.max_attempts = max_attempts
    rows, row0 = [], []
    for ll in lls:
        rows.append(np.full((2, ll.shape[1]), 7.0, ll.dtype))
        row0.append(sum(len(r) for r in rows))
        rows.append(ll)
    dev = torch.from_numpy(np.concatenate(rows)).to("cuda")
    out = capi.fb_batch(nets, [len(ll) for ll in lls], dev, row0, o)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_path_is_the_restatement_s(capi, model, case, force_global, dtype):
    name, text, T, seed = case
    net, rn = _net(capi, model, text)
    ll = HC.scores(T, S, seed).astype(dtype)
    want = RS.forward_backward(rn, ll.astype(np.float64), WIDE, WIDE, viterbi=True)
    assert want.status == RS.OK
    got = _run(capi, [net], [ll], force_global=force_global)[0]
    assert got["status"] == capi.FB_OK and got["shape"]["lds_form"] == (0 if force_global else 1)
    where = AR.engine_arcs(rn)
    assert got["path"].tolist() == [where[a] for a in want.path]
    slot, trslot = net.array("em_pdf"), net.array("em_tr")
    pdfs, trs = net.array("pdfs").tolist(), net.array("trs").tolist()
    counts = np.zeros(len(trs))
    for t, a in enumerate(got["path"]):
        assert got["pdf_occ"][t, pdfs.index(slot[a])] == 1.0 and got["pdf_occ"][t].sum() == 1.0
        counts[trs.index(trslot[a])] += 1
    assert (got["tr_occ"] == counts).all()
    plain = _run(capi, [net], [ll], want_path=False, force_global=force_global)[0]      # without want_path: the same bytes
    assert "path" not in plain and "path_refused" not in plain
    for k in ("status", "backward_total", "forward_total", "attempts"):
        assert plain[k] == got[k], k
    assert plain["pdf_occ"].tobytes() == got["pdf_occ"].tobytes() and plain["tr_occ"].tobytes() == got["tr_occ"].tobytes()


def test_a_retried_utterance_has_its_last_attempt_s_path_and_a_failed_one_is_refused(capi, model):
    """One batch: a chain that runs at once; the decoy network of tests/test_stats_bw_gpu.py's retry test, whose backward
    pass misses the initial node at beam W and reaches it at 2 W (W from the restatement's margins); a chain longer than
    its frames, which never runs."""
    T = 24
    ll = HC.scores(T, S, 311)
    order = np.argsort(ll.sum(axis=0))
    real = [int(order[0]), int(order[1]), int(order[2])]
    decoy = [int(ll[max(0, min(T - 1, T - 1 - k))].argmax()) for k in range(T + 4, -1, -1)]
    b = HC.Builder()
    init, fin = b.node(), b.node()
    for states in (real, decoy):
        nodes = [b.node() for _ in states]
        b.eps(init, nodes[0])
        for i, s in enumerate(states):
            b.emit(nodes[i], nodes[i], 2 * s)
            b.emit(nodes[i], nodes[i + 1] if i + 1 < len(states) else fin, 2 * s + 1)
    retry_net, retry_rn = _net(capi, model, b.text(init, fin))
    chosen = None
    for W in [round(10 * 1.12 ** k, 1) for k in range(40)]:
        r1 = RS.forward_backward(retry_rn, ll, WIDE, float(W), viterbi=True)
        r2 = RS.forward_backward(retry_rn, ll, WIDE, 2.0 * W, viterbi=True)
        if r1.status == RS.FAILED_BACKWARD and r2.status == RS.OK and min(r1.min_margin, r2.min_margin) >= 0.05:
            chosen = (W, r2)
            break
    assert chosen, "no backward beam separates the two attempts on this input"
    W, second = chosen
    ok_net, ok_rn = _net(capi, model, CASES[2][1])
    ok_ll = HC.scores(CASES[2][2], S, CASES[2][3])
    long_net, _ = _net(capi, model, HC.chain([s % S for s in range(T + 6)]))
    out = _run(capi, [ok_net, retry_net, long_net], [ok_ll, ll, HC.scores(T, S, 312)], bw=float(W), max_attempts=2)
    assert [o["attempts"] for o in out] == [1, 2, 2]
    assert out[1]["status"] == capi.FB_OK and out[1]["path"].tolist() == [AR.engine_arcs(retry_rn)[a] for a in second.path]
    first = RS.forward_backward(ok_rn, ok_ll, WIDE, float(W), viterbi=True)
    assert out[0]["path"].tolist() == [AR.engine_arcs(ok_rn)[a] for a in first.path]
    assert out[2]["status"] == capi.FB_FAILED_BACKWARD and "path" not in out[2]
    code, msg = out[2]["path_refused"]
    assert code == -1 and "did not run" in msg                     # AASR_ERR_INVALID


def test_a_batch_made_without_want_path_refuses_the_call(capi, model):
    import ctypes as C
    import torch
    L = capi.lib()
    name, text, T, seed = CASES[0]
    net, _ = _net(capi, model, text)
    dev = torch.from_numpy(HC.scores(T, S, seed)).to("cuda")
    o = capi.FbOptions.defaults()
    o.fw_beam = o.bw_beam = WIDE
    o.mode = capi.FB_VITERBI
    handles = (C.c_void_p * 1)(net.handle)
    frames, row0 = np.array([T], np.int32), np.array([0], np.int64)
    b = C.c_void_p()
    capi.check(L.aasr_fb_batch_create(C.byref(o), 1, handles, frames.ctypes.data, C.byref(b)))
    try:
        failed = C.c_int32(0)
        capi.check(L.aasr_fb_batch_dev(b, dev.data_ptr(), S, T, 1, row0.ctypes.data, 1, None))
        capi.check(L.aasr_fb_batch_sync(b, None, C.byref(failed)))
        arcs = np.full(T, -7, np.int32)
        assert L.aasr_fb_batch_path(b, 0, arcs.ctypes.data) == -1                 # AASR_ERR_INVALID
        assert "without want_path" in L.aasr_last_error().decode() and (arcs == -7).all()
    finally:
        L.aasr_fb_batch_destroy(b)

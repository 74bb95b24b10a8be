"""FstDecoder -- the reference's Python module of its FST decoder, on the engine.

The reference builds a SWIG module `FstDecoder` over decoder/src/FstSearch.hh; scripts do

    import FstDecoder
    s = FstDecoder.FstSearch("final.fst", "model.ph", "model.dur")
    s.set_beam(300); s.lna_open("a.lna", 1024); s.init_search(); s.run()
    print(s.get_result())

This module keeps the classes FstSearch, FstSearchC, FstConfidence and FstConfidenceWithPhoneLoop -- same method names,
argument order and meaning -- and runs the search on the device through the C ABI (include/aasr.h, aasr_fst_batch_*,
aasr_fst_conf_batch_*) as a batch of one utterance.  Strings are bytes, as the
reference's `bytestype`.  The .ph path is opened as the reference opens it (an unreadable file is the reference's
"FstAcoustics: open error") and otherwise unused: the search never consults the HMM file, the network carries the state
indices.  hmm_path and dur_path may be None.  The duration tables are indexed as the reference builds them unless
`dur_by_state` is set (csrc/fst_net.h).  Differences, on purpose: every lna_open starts at the file's first frame (the
reference never rewinds its frame counter), and a frame without any candidate ends the search with status NO_TOKENS and
the empty result where the reference indexes an empty vector.  The confidence classes: include/aasr.h, "FST decoder:
confidence", states the formulas and what is chosen where the reference is undefined (no end-node token, zero frames); the
reference's unconditional debug lines are not printed, its verbose block is when `verbose` is not 0.
`sys.path.insert(0, ".../aaltoasr_amd"); import FstDecoder` is the drop-in spelling.

lna_open_fd(fd, size) reads a descriptor -- a pipe that is still being written -- instead of a file: run() reads it in
blocks as they arrive and feeds each block to a one-session streaming search (capi.FstStream, include/aasr.h "FST
decoder: streaming sessions"), which is the batch search of the same frames bit for bit.  The confidence classes do the
same on a one-session streaming confidence (capi.FstConfStream, "FST decoder: confidence on streaming sessions").  A descriptor has no size to
derive the search's tables from: they are sized for STREAM_MAX_FRAMES frames (module level, settable before run(); a longer
input is refused when it gets there).  STREAM_BLOCK_FRAMES is the most frames one feed takes.
"""
import os
import struct

try:
    from . import capi as _A
except ImportError:  # imported as a top-level module named FstDecoder
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aaltoasr_amd import capi as _A


STREAM_MAX_FRAMES = 7500      # lna_open_fd: the longest input a descriptor may deliver (one minute at 125 frames/s)
STREAM_BLOCK_FRAMES = 64      # lna_open_fd: frames per feed at the most


def _guard(fn):
    def wrapped(*args, **kw):
        try:
            return fn(*args, **kw)
        except _A.AasrError as e:
            raise RuntimeError("Exception: %s" % e.msg) from None
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    wrapped.__wrapped__ = fn
    return wrapped


def _g(x) -> bytes:
    return (b"%g" % float(x))      # an ostream's default float format


class FstSearch:
    @_guard
    def __init__(self, search_fst_fname, hmm_path=None, dur_path=None):
        if hmm_path is not None:
            try:
                open(hmm_path, "rb").close()
            except OSError:
                raise RuntimeError("Exception: FstAcoustics: open error") from None
        self._dur = _A.FstDurations(dur_path) if dur_path is not None else None
        self._net = _A.FstNet(search_fst_fname)
        self._opt = _A.FstOptions.defaults()
        self._lna = None
        self._fd = None
        self._result = None
        self.verbose = 0
        self.dur_by_state = False
        self.status = _A.AASR_FST_OK

    def set_duration_scale(self, d):
        self._opt.duration_scale = d

    def set_beam(self, b):
        self._opt.beam = b

    def set_token_limit(self, t):
        self._opt.token_limit = t

    def set_transition_scale(self, t):
        self._opt.transition_scale = t

    def get_duration_scale(self):
        return self._opt.duration_scale

    def get_beam(self):
        return self._opt.beam

    def get_token_limit(self):
        return self._opt.token_limit

    def get_transition_scale(self):
        return self._opt.transition_scale

    def lna_open(self, file, size):
        """LnaReaderCircular::open: the 5-byte header, then the frames; `size` (the reader's buffer) is not needed"""
        try:
            data = open(file, "rb").read()
        except OSError:
            raise RuntimeError("Exception: LnaReaderCircular::open(): could not open %s" % file) from None
        if len(data) < 5:
            raise RuntimeError("Exception: LnaReaderCircular::read_int(): End of file reached.")
        n_models, lnabytes = struct.unpack(">iB", data[:5])
        if n_models <= 0:
            raise RuntimeError("Exception: LnaReaderCircular::open(): invalid number of states %d" % n_models)
        if lnabytes not in (1, 2, 4):
            raise RuntimeError("Exception: LnaReaderCircular::open(): invalid LNA byte number %d" % lnabytes)
        frames = (len(data) - 5) // (n_models * lnabytes)
        self._lna = (data[5:5 + frames * n_models * lnabytes], n_models, lnabytes, frames)

    def lna_open_fd(self, fd, size):
        """LnaReaderCircular::open_fd: the header from the descriptor now, the frames when run() reads them"""
        head = b""
        while len(head) < 5:
            piece = os.read(fd, 5 - len(head))
            if not piece:
                raise RuntimeError("Exception: LnaReaderCircular::read_int(): End of file reached.")
            head += piece
        n_models, lnabytes = struct.unpack(">iB", head)
        if n_models <= 0:
            raise RuntimeError("Exception: LnaReaderCircular::open(): invalid number of states %d" % n_models)
        if lnabytes not in (1, 2, 4):
            raise RuntimeError("Exception: LnaReaderCircular::open(): invalid LNA byte number %d" % lnabytes)
        self._lna = None
        self._fd = (fd, n_models, lnabytes)

    def lna_close(self):
        self._lna = None
        self._fd = None

    def _open_stream(self):
        """the one-session stream of _run_fd, and what reads its answer into the object"""
        self._opt.dur_by_state = 1 if self.dur_by_state else 0
        stream = _A.FstStream(self._net, 1, STREAM_MAX_FRAMES, self._opt, dur=self._dur)

        def take():
            self._result = stream.result(0)
        return stream, take

    def _run_fd(self):
        """the descriptor to its end: whole frames are fed as soon as they are there, at most STREAM_BLOCK_FRAMES a feed"""
        import torch
        fd, n_models, lnabytes = self._fd
        row = n_models * lnabytes
        stream, take = self._open_stream()
        try:
            held = b""
            while True:
                piece = os.read(fd, row * STREAM_BLOCK_FRAMES - len(held))
                held += piece
                frames = len(held) // row
                if frames:
                    d_lna = torch.frombuffer(bytearray(held[:frames * row] + bytes(16)), dtype=torch.uint8).cuda()
                    stream.feed_dev(d_lna, lnabytes, n_models, [0], [frames])
                    stream.sync()      # (d_lna is read by the queued launch: it must not be freed before)
                    held = held[frames * row:]
                if not piece:
                    break
            take()
        finally:
            stream.close()
        self.status = self._result["status"]

    def init_search(self):
        """one token at the initial node (FstSearch_tmpl.hh:45-51)"""
        self._result = {"status": _A.AASR_FST_OK, "tokens": [(self._net.initial, 0.0, 0, ())], "words": (), "text": b"",
                        "logprob": 0.0 if self._net.arrays()["node_end"][self._net.initial] else -1.0, "best_logprob": 0.0,
                        "best_final_logprob": 0.0 if self._net.arrays()["node_end"][self._net.initial] else -9999999.9}

    @_guard
    def run(self):
        if self._lna is None and self._fd is not None:      # (lna_open after lna_open_fd: the file, opened last)
            return self._run_fd()
        if self._lna is None:
            raise RuntimeError("Exception: LnaReaderCircular::go_to(): file not opened yet")
        import torch
        raw, n_models, lnabytes, frames = self._lna
        d_lna = torch.frombuffer(bytearray(raw + bytes(16)), dtype=torch.uint8).cuda()
        self._opt.dur_by_state = 1 if self.dur_by_state else 0
        self._result = _A.fst_batch(self._net, [frames], d_lna, lnabytes, n_models, [0], self._opt, dur=self._dur)[0]
        self.status = self._result["status"]

    def _need(self):
        if self._result is None:
            raise RuntimeError("Exception: init_search() or run() first")
        return self._result

    def get_result(self):
        return self._need()["text"]

    def get_result_and_logprob(self):
        r = self._need()
        return r["text"], float(r["logprob"])

    def get_best_token_logprob(self):
        return float(self._need()["best_logprob"])

    def get_best_final_token_logprob(self):
        return float(self._need()["best_final_logprob"])

    def _token(self, t) -> bytes:
        node, lp, dur, words = t
        return b"Token %d %s dur %d '%s '" % (node, _g(lp), dur, b"".join(b" " + self._net.symbols[w] for w in words))

    def tokens_at_final_states(self):
        end = self._net.arrays()["node_end"]
        return b"Tokens at final nodes:\n" + b"".join(b"  " + self._token(t) + b"\n" for t in self._need()["tokens"] if end[t[0]])

    def best_tokens(self, n=10):
        """the reference's loop prints n + 2 tokens at the most (`if (c++ > n) break` after the print)"""
        return b"Best tokens:\n" + b"".join(b"  " + self._token(t) + b"\n" for t in self._need()["tokens"][:n + 2])


class FstSearchC(FstSearch):
    """the reference's second instantiation of its search template (FstSearch_base<FstConfidenceToken>): FstSearch's surface"""


class FstConfidence(FstSearchC):
    """FstConfidence(grammar_fst, hmm, dur): the grammar search and a confidence, 0.5 * (token_conf + best_acu_conf).
    The reference's run() computes every frame's best acoustic value here and discards it: the sum is unused in this
    class, best_acu_score stays 0, and the frame-best pass is not run."""
    _phone_loop = 0

    @_guard
    def __init__(self, grammar_fst_name, hmm_fname=None, dur_fname=None):
        FstSearch.__init__.__wrapped__(self, grammar_fst_name, hmm_fname, dur_fname)
        self._phone_net = None
        self._phone_opt = _A.FstOptions.defaults()
        self._conf = None
        self._logprob_conf_weight = 2.0            # set and never read, as in the reference
        self._logprob_conf_hysteresis = 100.0

    def set_logprob_conf_weight(self, lpw):
        self._logprob_conf_weight = lpw

    def set_logprob_conf_hysteresis(self, h):
        self._logprob_conf_hysteresis = h

    def init_search(self):
        """both searches back to one token at their initial nodes"""
        FstSearch.init_search(self)
        self._conf = None

    def _conf_options(self):
        self._opt.dur_by_state = self._phone_opt.dur_by_state = 1 if self.dur_by_state else 0
        o = _A.FstConfOptions.defaults(phone_loop=self._phone_loop, verbose=0)
        o.grammar, o.phone = self._opt, self._phone_opt
        return o

    def _open_stream(self):
        """a one-session confidence stream (capi.FstConfStream): the batch confidence of the same frames bit for bit"""
        stream = _A.FstConfStream(self._net, self._phone_net, 1, STREAM_MAX_FRAMES, self._conf_options(), dur=self._dur)

        def take():
            self._conf = stream.result(0, want_tokens=True)
            self._result = self._conf["grammar"]
        return stream, take

    @_guard
    def run(self):
        if self._lna is None and self._fd is not None:      # (lna_open after lna_open_fd: the file, opened last)
            return self._run_fd()
        if self._lna is None:
            raise RuntimeError("Exception: LnaReaderCircular::go_to(): file not opened yet")
        import torch
        raw, n_models, lnabytes, frames = self._lna
        d_lna = torch.frombuffer(bytearray(raw + bytes(16)), dtype=torch.uint8).cuda()
        o = self._conf_options()
        self._conf = _A.fst_conf_batch(self._net, self._phone_net, [frames], d_lna, lnabytes, n_models, [0], o, dur=self._dur,
                                       want_tokens=True)[0]
        self._result = self._conf["grammar"]
        self.status = self._result["status"]

    def _need_conf(self):
        if self._conf is None:
            raise RuntimeError("Exception: run() first")
        if not self._conf["valid"]:
            raise RuntimeError("Exception: the search overflowed a capacity (%s, %s)" % (
                _A.FST_STATUS_NAMES[self._conf["grammar_status"]], _A.FST_STATUS_NAMES[self._conf["phone_status"]]))
        return self._conf

    def result_and_confidence(self):
        """(result string, confidence)"""
        c = self._need_conf()
        if self.verbose and self._phone_loop:
            import sys
            sys.stderr.write("%s:\n\tToken: %.4f\n\tPloop: %.4f\n\tEdit: %.4f\n\tBacu: %.4f\n\tTotal: %.4f\n\n" % (
                c["text"].decode("latin-1"), c["token_conf"], c["ploop_conf"], c["edit_conf"], c["best_acu_conf"], c["confidence"]))
        return c["text"], float(c["confidence"])


class FstConfidenceWithPhoneLoop(FstConfidence):
    """FstConfidenceWithPhoneLoop(grammar_fst, phone_loop_fst, hmm, dur): a second search over the phone-loop network on
    the same acoustics; the confidence weighs the phone-loop, token, edit-distance and best-acoustics terms (1, 20, 5, 1)."""
    _phone_loop = 1

    @_guard
    def __init__(self, grammar_fst_name, phone_loop_fst_name, hmm_fname=None, dur_fname=None):
        FstConfidence.__init__.__wrapped__(self, grammar_fst_name, hmm_fname, dur_fname)
        self._phone_net = _A.FstNet(phone_loop_fst_name)
        self._ploop_logprob_weight = 0.8           # set and never read, as in the reference

    def set_phone_beam(self, pb):
        self._phone_opt.beam = pb

    def set_phone_token_limit(self, ptl):
        self._phone_opt.token_limit = int(ptl)

    def set_phone_duration_scale(self, pds):
        self._phone_opt.duration_scale = pds

    def set_phone_loop_logprob_weight(self, w):
        self._ploop_logprob_weight = w

    def get_ploop_conf(self):
        return float(self._need_conf()["ploop_conf"])

    def get_token_conf(self):
        return float(self._need_conf()["token_conf"])

    def get_edit_conf(self):
        return float(self._need_conf()["edit_conf"])

    def get_best_acu_conf(self):
        return float(self._need_conf()["best_acu_conf"])

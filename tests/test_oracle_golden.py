"""CPU tests that PIN THE ORACLE: against the reference's own golden files
(aku/tests/*.ref with short.wav and the .feaconf files, copied as data under
tests/golden/), against the real KissFFT / util.hh / ModuleConfig where
oracle/_ref was built (KissFFT, util.hh and the LNA reader elsewhere against
their outputs recorded in tests/golden/reference_outputs.npz), and against
hand-derived expectations of the text formats.  No GPU, no product code."""
import ctypes as C
import os

import numpy as np
import pytest


def _make_golden():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_golden.py")
    spec = importlib.util.spec_from_file_location("make_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


make_golden = _make_golden()     # the pins' inputs, shared with the tool that records the reference's outputs


@pytest.fixture(scope="module")
def recorded(golden_dir):
    """What the reference's own code returned on the pins' inputs (tools/make_golden.py --reference): the pins
    below compare with it where oracle/_ref was not built."""
    return np.load(os.path.join(golden_dir, "reference_outputs.npz"))


def _load(oracle, golden_dir, name):
    pcm, sr = oracle.read_wav_pcm16(os.path.join(golden_dir, "short.wav"))
    assert sr == 16000 and len(pcm) == 9506
    ch = oracle.FeatureChain(open(os.path.join(golden_dir, name + ".feaconf")).read())
    ref = np.loadtxt(os.path.join(golden_dir, name + ".ref"))
    return pcm, ch, ref


def test_mfcc_p_dd_matches_reference_golden(oracle, golden_dir):
    """aku/tests/mfcc_p_dd.script: feacat --start-frame -10 --end-frame 80,
    twice (second pass from the round-tripped config) -> 182 x 39 values
    printed with two decimals."""
    pcm, ch, ref = _load(oracle, golden_dir, "mfcc_p_dd")
    assert ch.dim == 39 and ref.shape == (182, 39)
    assert ch.last_frame(len(pcm)) == 72
    fea = ch.generate(pcm, -10, 91)
    assert np.abs(fea - ref[:91]).max() <= 0.005 + 1e-9
    assert np.abs(fea - ref[91:]).max() <= 0.005 + 1e-9


def test_mfcc_cms_norm_matches_reference_golden(oracle, golden_dir):
    """aku/tests/mfcc_cms_norm.script: frames -15..90 through normalization,
    39x39 lin_transform and the 50/25 mean subtractor."""
    pcm, ch, ref = _load(oracle, golden_dir, "mfcc_cms_norm")
    assert ref.shape == (106, 39)
    assert ch.halo() == (55, 30)
    fea = ch.generate(pcm, -15, 106)
    assert np.abs(fea - ref).max() <= 0.005 + 1e-9


def test_random_access_is_deterministic(oracle, golden_dir):
    """aku/tests/random_feature_test.cc: re-requesting frames in random order
    must reproduce the sequential values (here: to 1e-12, the only
    order-dependent piece being the mean subtractor's running update)."""
    pcm, ch, _ = _load(oracle, golden_dir, "mfcc_cms_norm")
    seq = ch.generate(pcm, -10, 91)
    rng = np.random.default_rng(1)
    for f in rng.integers(-10, 81, 40):
        one = ch.generate(pcm, int(f), 1)
        assert np.abs(one[0] - seq[f + 10]).max() < 1e-12


def test_fft_bit_exact_vs_reference_kissfft(oracle, recorded):
    """The oracle's real FFT against KissFFT's kiss_fftr, bit for bit: live where oracle/_ref holds the reference's
    build, else against the SHA-256 of every output the reference produced on the same inputs."""
    K = oracle.ref_kissfft()
    L = oracle.lib()
    pf = C.POINTER(C.c_float)
    # the last six sizes need the generic butterfly (prime factors 7, 11, 13, 17, 23 of the half length)
    cfgs = {}
    sha = recorded["kissfft_sha256"].reshape(-1, 32)
    for i, (n, x) in enumerate(make_golden.fft_inputs()):
        re = np.zeros(n // 2 + 1, np.float32)
        im = np.zeros(n // 2 + 1, np.float32)
        assert L.orc_rfft(n, x.ctypes.data_as(pf), re.ctypes.data_as(pf), im.ctypes.data_as(pf)) == 0
        if K is None:
            mine = np.empty((n // 2 + 1) * 2, np.float32)
            mine[0::2], mine[1::2] = re, im
            assert np.array_equal(make_golden.digest(mine), sha[i]), (n, i % make_golden.FFT_REPS)
            continue
        cfg = cfgs.setdefault(n, K.kiss_fftr_alloc(n, 0, None, None))
        out = np.zeros((n // 2 + 1) * 2, np.float32)
        K.kiss_fftr(cfg, x.ctypes.data_as(pf), out.ctypes.data_as(pf))
        assert np.array_equal(out[0::2].view(np.uint32), re.view(np.uint32))
        assert np.array_equal(out[1::2].view(np.uint32), im.view(np.uint32))


def test_safe_log_and_str2float_vs_reference(oracle, recorded):
    A = oracle.ref_aku()
    L = oracle.lib()
    ok = C.c_int()
    for x, want in zip(make_golden.SAFE_LOG_ARGS, recorded["safe_log"]):
        assert (A.ref_safe_log(x) if A is not None else want) == L.orc_safe_log(x)
    for s, want in zip(make_golden.STR2FLOAT_ARGS, recorded["str2float"]):
        assert np.float32(A.ref_str2float(s.encode(), C.byref(ok)) if A is not None else want) == oracle.str2float(s)


def test_module_config_parser_vs_reference(oracle, golden_dir):
    """The reference's ModuleConfig::read + typed get on the real feaconf."""
    A = oracle.ref_aku()
    if A is None:
        pytest.skip("oracle/_ref/libaku_ref.so not built (no reference tree)")
    path = os.path.join(golden_dir, "mfcc_cms_norm.feaconf")
    text = open(path).read()
    mods = oracle.parse_feature_config(text)
    assert [m["name"] for m in mods][:4] == ["audiofile", "fft", "mel", "power"]
    # walk the file with the reference parser, block by block
    offset = 0
    raw = open(path, "rb").read()
    buf = C.create_string_buffer(1 << 16)
    new_off = C.c_long()
    for m in mods:
        offset = raw.index(b"module", offset) + len(b"module")
        offset = raw.index(b"\n", offset) + 1
        n = A.ref_module_config_read(path.encode(), offset, buf, len(buf), C.byref(new_off))
        assert n > 0, buf.value
        block = buf.value.decode()
        ref_opts = {}
        for ln in block.splitlines():
            ln = ln.strip()
            if ln in ("{", "}", ""):
                continue
            k, v = ln.split(None, 1)
            ref_opts[k] = v
        assert ref_opts == m
        for key in ("mean", "scale", "matrix"):
            if key in m:
                out = np.zeros(2048, np.float32)
                cnt = A.ref_module_config_get_floats(block.encode(), key.encode(),
                                                     out.ctypes.data_as(C.POINTER(C.c_float)), 2048)
                mine = np.array([oracle.str2float(x) for x in m[key].split()], np.float32)
                assert cnt == len(mine)
                assert np.array_equal(out[:cnt], mine)
        offset = new_off.value


def test_diag_gaussian_matches_textbook_logpdf(oracle):
    """Independent cross-check of the scoring restatement: the reference omits
    (2*pi)^(-d/2), so ll + d/2*log(2*pi) must equal the normal log-density."""
    from scipy.stats import norm
    rng = np.random.default_rng(3)
    D, G = 7, 5
    mean = rng.standard_normal((G, D))
    var = np.exp(rng.uniform(-1, 1, (G, D)))
    m = oracle.DiagModel(mean, var, np.arange(G + 1, dtype=np.int32), np.arange(G, dtype=np.int32), np.ones(G))
    x = rng.standard_normal((4, D))
    ll = m.gauss_loglik(x)
    for f in range(4):
        for g in range(G):
            want = norm.logpdf(x[f], mean[g], np.sqrt(var[g])).sum() + 0.5 * D * np.log(2 * np.pi)
            assert abs(ll[f, g] - want) < 1e-10


def test_mixture_and_floor(oracle):
    mean = np.zeros((2, 1))
    var = np.ones((2, 1))
    m = oracle.DiagModel(mean, var, [0, 2], [0, 1], [3.0, 1.0])
    assert np.allclose(m.mix_w, [0.75, 0.25])           # Mixture::normalize_weights
    assert abs(m.score(np.array([[0.0]]))[0, 0]) < 1e-12  # lik 1 -> log 0
    far = m.score(np.array([[40.0]]))[0, 0]
    assert far == np.log(1e-50)                            # HmmSet 1e-50 clamp


def test_invalid_gaussian_constant(oracle):
    """var <= 0 -> precision 0 -> product 0 -> constant stays 0."""
    m = oracle.DiagModel(np.zeros((1, 2)), np.array([[1.0, 0.0]]), [0, 1], [0], [1.0])
    assert m.cst[0] == 0.0 and m.prec[0, 1] == 0.0
    assert abs(m.gauss_loglik(np.array([[2.0, 5.0]]))[0, 0] - (-2.0)) < 1e-12


def test_lna_encoding_rules(oracle):
    lik = np.array([[0.5, 0.25, 0.25, 1e-60, 3e-46, 1e-20]])
    lp, by = oracle.lna_encode(lik, True, 2)
    z = np.float32(0.5) + np.float32(0.25) * 2 + np.float64(np.float32(3e-46)) + np.float64(np.float32(1e-20))
    assert lp[0, 0] == np.float32(np.log(np.float32(0.5) / z))
    assert lp[0, 3] == np.float32(np.log(1e-50))           # float flush -> safe_log floor
    code = by[0].reshape(-1, 2).astype(int)
    assert list(code[0]) == [(int(-1820.0 * float(lp[0, 0]) + .5) >> 8) & 255, int(-1820.0 * float(lp[0, 0]) + .5) & 255]
    assert list(code[3]) == [255, 255] and list(code[5]) == [255, 255]
    lp4, by4 = oracle.lna_encode(lik, False, 4)
    assert lp4[0, 1] == np.float32(np.log(np.float32(0.25)))
    assert np.array_equal(by4.view("<f4")[0], lp4[0])
    # all states zero -> Z forced to 1, everything at the floor
    lp0, _ = oracle.lna_encode(np.zeros((1, 3)), True, 2)
    assert np.all(lp0 == np.float32(np.log(1e-50)))
    assert oracle.lna_header(3125, 2) == bytes([0, 0, 0x0c, 0x35, 2])
    dec = oracle.lna_decode(oracle.lna_header(6, 2) + by.tobytes())
    assert np.abs(dec[0, :3] - lp[0, :3]).max() < 1 / 1820.0


def test_recipe_batches_partition_the_lines(oracle):
    """Recipe::read: contiguous slices, first (L mod n) batches one longer."""
    for L in range(1, 26):
        text = "\n".join("audio=a%d.wav lna=a%d.lna" % (i, i) for i in range(L)) + "\n"
        for n in range(1, 9):
            seen = []
            sizes = []
            for b in range(1, n + 1):
                infos = oracle.recipe_read(text, n, b)
                sizes.append(len(infos))
                seen += [i.audio_path for i in infos]
            if n <= L:
                assert seen == ["a%d.wav" % i for i in range(L)], (L, n)
                assert max(sizes) - min(sizes) <= 1
                assert sizes == sorted(sizes, reverse=True)
    assert len(oracle.recipe_read("# c\n\naudio=x lna=y start-time=1.5 end-time=2\n")) == 1


def test_recipe_keys_persist_across_lines(oracle):
    """aku/Recipe.cc never clears its key map between lines."""
    infos = oracle.recipe_read("audio=a.wav lna=a.lna speaker=s1\naudio=b.wav lna=b.lna\n")
    assert infos[1].speaker_id == "s1"
    with pytest.raises(ValueError):
        oracle.recipe_read("audio=a=b\n")


def test_model_files_roundtrip(oracle, tmp_path):
    from aaltoasr_amd import synth
    mean, var, off, idx, w = synth.make_model(D=5, G=12, S=4, comps=3, seed=4)
    base = str(tmp_path / "m")
    oracle.write_gk(base + ".gk", mean, var)
    oracle.write_mc(base + ".mc", off, idx, w)
    m = oracle.read_model(base)
    assert np.array_equal(m.mean, mean) and np.array_equal(m.var, var)
    assert np.array_equal(m.mix_idx, idx) and np.allclose(m.mix_w, w)
    oracle.write_gk(base + "_legacy.gk", mean, var, legacy=True)
    m2, v2 = oracle.read_gk(base + "_legacy.gk")
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)


def test_config_errors(oracle):
    with pytest.raises(ValueError, match="Unknown module type"):
        oracle.FeatureChain("module\n{\n name a\n type nosuch\n}\n")
    with pytest.raises(ValueError, match="first module"):
        oracle.FeatureChain("module\n{\n name a\n type fft\n}\n")
    with pytest.raises(ValueError, match="Must set sample rate"):
        oracle.FeatureChain("module\n{\n name a\n type audiofile\n}\n")
    with pytest.raises(ValueError, match="sources not defined"):
        oracle.FeatureChain("module\n{\n name a\n type audiofile\n sample_rate 16000\n}\nmodule\n{\n name f\n type fft\n}\n")
    ch = oracle.FeatureChain("module\n{\n name a\n type audiofile\n sample_rate 16000\n}\n")
    with pytest.raises(ValueError, match="audio shorter than frame"):
        ch.generate(np.zeros(100, np.int16), 0, 1)


def test_clustering_oracle_properties(oracle, tmp_path):
    """The restatement of PDFPool's cluster branch (no reference goldens exist for
    it): evaluating every cluster == plain scoring; evaluating none == every
    Gaussian replaced by its centre; the .gcl reader repeats the last pair; the
    heap pops best-first."""
    from aaltoasr_amd import synth
    mean, var, off, idx, w = synth.make_model(D=12, G=300, S=30, comps=10)
    g2c = synth.make_clustering(mean, 20)
    om = oracle.DiagModel(mean, var, off, idx, w)
    frames = synth.make_frames(40, D=12).astype(np.float64)
    exact = om.score(frames)
    pairs = [(g, int(c)) for g, c in enumerate(g2c)]
    om.set_clustering(20, pairs, 1.0, 1.0)
    assert om.min_clusters == 20 and om.min_gaussians == 300
    s_all, n_all = om.score_clustered(frames, want_counts=True)
    assert np.array_equal(s_all, exact) and (n_all == 20).all()
    om.set_clustering(20, pairs, 0.0, 0.0)
    s_none, n_none = om.score_clustered(frames, want_counts=True)
    assert (n_none == 0).all()
    # every Gaussian stands for its centre: rebuild that model by hand
    c_var = np.where(om.c_prec > 0, 1.0 / np.where(om.c_prec > 0, om.c_prec, 1.0), 0.0)
    sub = oracle.DiagModel(om.c_mean[g2c], c_var[g2c], off, idx, w)
    assert np.abs(sub.score(frames) - s_none).max() < 1e-9
    # monotone in the thresholds: more exact clusters never fewer
    om.set_clustering(20, pairs, 0.0, 0.2)
    n20 = om.score_clustered(frames, want_counts=True)[1]
    om.set_clustering(20, pairs, 0.0, 0.5)
    n50 = om.score_clustered(frames, want_counts=True)[1]
    assert (n50 >= n20).all() and (n20 >= 1).all()
    # centre = unit-weight moment match of its members
    c = 3
    mem = np.flatnonzero(g2c == c)
    assert np.allclose(om.c_mean[c], mean[mem].mean(0), rtol=1e-13)
    want_var = (var[mem] + mean[mem] ** 2).mean(0) - mean[mem].mean(0) ** 2
    assert np.allclose(1.0 / om.c_prec[c], want_var, rtol=1e-11)
    # reader: last pair twice, "insensible" cluster counts refused like the reference
    path = str(tmp_path / "x.gcl")
    oracle.write_gcl(path, 20, g2c)
    n, rp = oracle.read_gcl(path, 300)
    assert n == 20 and rp[:-1] == pairs and rp[-1] == pairs[-1]
    with pytest.raises(ValueError, match="insensible"):
        oracle.read_gcl(path, 60)


def test_speaker_config_oracle(oracle):
    """The SpeakerConfig restatement on the CPU: module order, defaults for unknown
    speakers, the "%g" read-back of a repeated speaker, stale model transforms."""
    cfg = ("module\n{\n name a\n type audiofile\n sample_rate 16000\n}\n"
           "module\n{\n name f\n type fft\n sources a\n}\nmodule\n{\n name v\n type vtln\n sources f\n}\n"
           "module\n{\n name m\n type mel\n sources v\n}\nmodule\n{\n name n\n type normalization\n sources m\n}\n")
    ch = oracle.FeatureChain(cfg)
    from aaltoasr_amd import synth
    om = oracle.DiagModel(*synth.make_model(D=21, G=40, S=4, comps=10))
    w = np.hstack([np.zeros((21, 1)), np.eye(21)])
    w[0, 0] = 0.123456789
    text = ("speaker default\n{\n v\n {\n }\n}\n"
            "speaker s1\n{\n feature v\n {\n  warp_factor 1.0123456\n }\n model cmllr\n {\n  unitmode UNIT_MIX\n"
            "  w1 1 2 %s\n }\n}\n" % " ".join("%.9g" % x for x in w.ravel()))
    sc = oracle.SpeakerConfig(ch, om)
    sc.read_text(text)
    sc.set_speaker("s1")
    assert float(ch.by_name["v"].prm["warp"]) == float(np.float32(1.0123456))
    assert set(np.flatnonzero(sc.g2t >= 0)) == set(range(10, 30))
    assert sc.W[0][0, 0] == float(np.float32(0.123456789))       # str2float
    sc.set_speaker("s1")                                           # read back through "%g"
    assert float(ch.by_name["v"].prm["warp"]) == float(np.float32(1.01235))
    assert sc.speakers["s1"]["model cmllr"]["w1"].split()[2] == "0.123457"
    sc.set_speaker("nobody")                                       # defaults; cmllr block absent:
    assert float(ch.by_name["v"].prm["warp"]) == 1.0               # the previous transform stays loaded
    assert set(np.flatnonzero(sc.g2t >= 0)) == set(range(10, 30)) and "nobody" in sc.speakers
    with pytest.raises(ValueError, match="Default utterance is required"):
        sc.set_utterance("")
    with pytest.raises(ValueError, match="Syntax error"):
        oracle.SpeakerConfig(ch).read_text("spk x\n{\n}\n")


def test_pre_module_golden(oracle, golden_dir):
    """aku/tests/pre_test.script on the oracle: frames 10..60 of the mfcc_p_dd chain written
    as float32 and read back through pre.feaconf == aku/tests/pre_test.ref (two decimals)."""
    pcm, _ = oracle.read_wav_pcm16(os.path.join(golden_dir, "short.wav"))
    src = oracle.FeatureChain(open(os.path.join(golden_dir, "mfcc_p_dd.feaconf")).read())
    feats = src.generate(pcm, 10, 51).astype(np.float32)
    pre = oracle.FeatureChain(open(os.path.join(golden_dir, "pre.feaconf")).read())
    assert pre.dim == 39 and pre.last_frame(feats.size) == 50
    out = pre.generate(feats, 0, 51)
    ref = np.loadtxt(os.path.join(golden_dir, "pre_test.ref"))
    assert np.abs(out - ref).max() <= 0.005 + 1e-9
    assert np.array_equal(pre.generate(feats, -2, 2), np.repeat(out[:1], 2, 0))
    assert np.array_equal(pre.generate(feats, 51, 3), np.repeat(out[-1:], 3, 0))


@pytest.mark.parametrize("nbytes", [2, 4])
def test_lna_files_read_by_the_reference_decoder_reader(oracle, recorded, tmp_path, nbytes):
    """The consumer side of the LNA format, pinned on the real reference code: a file written
    by the oracle's phone_probs restatement (aku/phone_probs.cc:213-262) is opened with the
    recogniser's own LnaReaderCircular (decoder/src/LnaReaderCircular.cc, compiled in place) and
    its log_prob() view is (a) what the oracle's lna_decode says and (b) within the format's
    resolution of the log-probabilities phone_probs computed.  Where oracle/_ref was not built, the reader's
    output on the same file as recorded by tools/make_golden.py --reference."""
    path = str(tmp_path / "x.lna")
    F, S, lp = make_golden.lna_pin_file(path, nbytes)
    live = oracle.ref_lna() is not None
    if not live:
        assert np.array_equal(make_golden.digest(np.frombuffer(open(path, "rb").read(), np.uint8)),
                              recorded["lna%d_file_sha256" % nbytes]), "the oracle writes another file than the one recorded"
    for k, (order, buf) in enumerate(make_golden.LNA_READS):
        got = oracle.ref_lna_read(path, F + 5, S, buf_size=buf, order=order) if live else recorded["lna%d_reads" % nbytes][k]
        assert got.shape == (F, S)       # go_to() reports EOF exactly after the last frame
        want = oracle.lna_decode(open(path, "rb").read())
        assert np.array_equal(got, want.astype(np.float32))
    if nbytes == 4:
        assert np.array_equal(got, lp)
    else:
        inside = lp > -36.0
        assert np.abs(got - lp)[inside].max() <= 0.5 / 1820 + 1e-6
        assert np.all(got[~inside] <= -36.0)


def test_eof_frame_is_where_a_sequential_reader_meets_the_end(oracle):
    """orc_eof_frame against the definition (first frame whose window [ws, ws + width + 1), ws =
    (int)(float(frame) * advance), crosses the end; aku/FeatureModules.cc:399-413) by brute force:
    integral and fractional advances, lengths around 2^24 samples where last_frame()'s float formula
    goes off by one."""
    L = oracle.lib()
    rng = np.random.default_rng(12)
    cases = [(128.0, 256), (160.0, 400), (110.25, 220), (220.5, 442), (441.0, 1000), (88.2, 200), (64.0, 128)]
    differs = 0
    for adv, width in cases:
        adv32 = np.float32(adv)
        lens = list(rng.integers(width + 1, 200000, 60)) + list(rng.integers((1 << 24) - 3000, (1 << 24) + 300000, 40)) \
            + [57600000, width + 1, width + 2]
        for n in lens:
            n = int(n)
            got = L.orc_eof_frame(n, width, float(adv32))
            f = max(0, got - 3)
            while int(np.float32(f) * adv32) + width + 1 <= n:
                f += 1
            assert got == f, (adv, width, n, got, f)
            assert int(np.float32(max(got - 1, 0)) * adv32) + width + 1 <= n or got == 0
            differs += got != L.orc_last_frame(n, width, float(adv32)) + 1
    assert differs > 0          # the two do part ways (fractional advances, long files)
    assert L.orc_eof_frame(100, 256, 128.0) == 0

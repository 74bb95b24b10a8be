"""The three training drivers see the same frames through the shared recipe pass (csrc/recipe_pass.cc): one recipe of
four short utterances -- one with start-time / end-time, one whose .phn cannot be initialised (an empty file), one whose
segmentation runs past the audio's end -- no speaker file for stats and lda, through run_stats_recipe, run_lda_recipe and
run_mllr_recipe (every line under one speaker).

* stats' per-state frame count (the .gks feacount of the state's own Gaussians: an untied model whose Gaussians lie
  among the frames, so that every frame has a positive total) and lda's state_gamma (--mingamma 1: every state with a
  frame is selected) are sums of ones in double: equal, exactly, and equal to the counts taken on the host from
  aasr_stats_read_segmentation over the same files with the same frame limits.
* the frames in aasr_run_stats of all three runs are that total.

All four utterances take part: frames past the feature end are cut by the segmentation reader for the three tools
alike, and the utterance without a segmentation adds nothing anywhere."""
import numpy as np
import pytest

from aaltoasr_amd import synth
from test_lda_gpu import LABELS, PER, TD, lda_config, random_phn, write_ph, write_wav
from test_stats_gpu import read_gks

pytestmark = pytest.mark.gpu

COMPS = 2
TIMES = {1: (0.2, 0.9)}     # recipe line -> start-time, end-time


@pytest.fixture(scope="module")
def setup(capi, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("pass")
    lda_text = lda_config()
    cfg_text = lda_text[:lda_text.index("module\n{\n  name lda")]     # the chain the lda module reads: stats and mllr end there
    ft = capi.Feat(cfg_text)
    open(str(d / "f.cfg"), "w").write(cfg_text)                       # (for running the tools on this directory by hand)
    open(str(d / "lda.cfg"), "w").write(lda_text)
    write_ph(str(d / "m.ph"))
    rng = np.random.default_rng(29)
    lines, utts = [], []
    for u in range(4):
        pcm = synth.make_audio(16000 + 3000 * u, seed=400 + u)
        wav, phn = str(d / ("u%d.wav" % u)), str(d / ("u%d.phn" % u))
        write_wav(wav, pcm)
        eof = ft.eof_frame(len(pcm))
        if u == 2:
            open(phn, "w").close()                                    # no line: the segmentation cannot be initialised
        else:
            random_phn(phn, rng, eof + 30 if u == 3 else eof - 25)
        # recipe keys persist across lines (aku/Recipe.cc): every line sets its times
        lines.append("audio=%s transcript=%s alignment=%s speaker=s1 start-time=%g end-time=%g"
                     % ((wav, phn, phn) + TIMES.get(u, (0, 0))))
        utts.append(dict(pcm=pcm, phn=phn, eof=eof))
    open(str(d / "r.rcp"), "w").write("\n".join(lines) + "\n")
    # an untied model whose Gaussians lie among the frames
    S, D = len(LABELS) * PER, ft.dim
    fea = np.concatenate([ft.run(x["pcm"], 0, x["eof"], dtype=np.float64) for x in utts])
    mean, var, off, idx, w = synth.make_model(D=D, G=COMPS * S, S=S, comps=COMPS, seed=31)
    mean[:] = fea[rng.integers(0, len(fea), len(mean))] + 0.3 * rng.standard_normal(mean.shape)
    var[:] = rng.uniform(0.5, 2.0, var.shape)
    oracle.write_gk(str(d / "m.gk"), mean, var)
    oracle.write_mc(str(d / "m.mc"), off, idx, w)
    topo = capi.Topology(str(d / "m.ph"))
    # the host's counts, through the exported segmentation reader
    fr = np.float32(ft.frame_rate)
    count = np.zeros(S)
    for u, x in enumerate(utts):
        first, last = (int(np.float32(t) * fr) for t in TIMES.get(u, (0, 0)))
        seg = capi.stats_read_segmentation(topo, x["phn"], ft.frame_rate, first, last, x["eof"], False)
        assert (seg is None) == (u == 2)
        if seg is not None:
            assert (seg[2] == -1).all()                               # no transitions asked for: none reported
            count += np.bincount(seg[1], minlength=S)
    assert count.sum() > 0 and (count > 0).sum() >= TD + 1
    return dict(dir=d, cfg_text=cfg_text, lda_text=lda_text, topo=topo, count=count, off=off, idx=idx, S=S)


def test_stats_lda_and_mllr_count_the_same_frames(capi, setup, tmp_path):
    st, d = setup, setup["dir"]
    rcp, count = str(d / "r.rcp"), setup["count"]
    gmm = lambda: capi.Gmm.from_files(str(d / "m.gk"), str(d / "m.mc"), str(d / "m.ph"))
    ft = capi.Feat(st["cfg_text"])

    res_stats = capi.run_stats_recipe(ft, gmm(), st["topo"], rcp, str(tmp_path / "s"))
    gks = read_gks(str(tmp_path / "s.gks"))[1]
    stats_count = np.array([gks[int(st["idx"][st["off"][s]])][0] if int(st["idx"][st["off"][s]]) in gks else 0
                            for s in range(st["S"])], np.float64)

    res_lda = capi.run_lda_recipe(st["lda_text"], st["topo"], rcp, "lda", TD, opts=capi.LdaOptions.defaults(mingamma=1.0))

    g = gmm()
    sc = capi.SpeakerConfig(ft, g)
    sc.read_text("speaker default\n{\n  model cmllr\n  {\n  }\n}\n")
    res_mllr = capi.run_mllr_recipe(ft, g, st["topo"], rcp, sc)

    print("frames: host %d, stats %d, lda %d, mllr %d; states with frames %d" %
          (count.sum(), res_stats["frames"], res_lda["frames"], res_mllr["frames"], (count > 0).sum()))
    assert (stats_count == count).all()
    assert (res_lda["state_gamma"] == count).all()
    assert res_stats["frames"] == res_lda["frames"] == res_mllr["frames"] == count.sum()
    assert res_stats["utterances"] == res_lda["utterances"] == res_mllr["utterances"] == 4
